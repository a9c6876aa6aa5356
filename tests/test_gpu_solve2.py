"""The tracker's 2x2 solve on two lanes against the wave-uniform solve
(csrc/track7_solve.h, through klt_hip_selftest_solve2).

k_track7's pass computes dx in lane 0 and dy in lane 1 with one instruction
stream; each lane runs the uniform solve's operations on its operands, so the
two must agree on every input bit for bit -- NaNs included, whose payloads
follow the operand order.  The hook runs, per case, the uniform solve, the
two-lane solve from the ordered sums' lanes (the exact instances) and the
two-lane solve from uniform sums (the fast-sum instances).

Cases: the level-0 window sums of scene 7's placed list over its thirteen frame
pairs (numpy, float32: realistic magnitudes, flat windows on the plate), 2^16
random bit patterns, and a set of special values -- denormals, zeros of both
signs, infinities, and determinants just below, at and just above min_det.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import motion_scenes as ms

pytestmark = pytest.mark.gpu

F32 = np.float32
MIN_DET = F32(0.01)  # the tracking context's default min_determinant


def scene_sums():
    """{gxx, gxy, gyy, sum(dif gx), sum(dif gy)} of the 7x7 windows at the placed
    list's (truncated) positions, every frame pair of scene 7; float32 throughout."""
    fr = [f.astype(F32) for f in ms.scene(7)]
    x, y, _ = ms.placed_list()
    xi, yi = x.astype(int), y.astype(int)
    rows = []
    for a, b in zip(fr[:-1], fr[1:]):
        gy, gx = np.gradient(a + b)
        dif = a - b
        for cx, cy in zip(xi, yi):
            w = np.s_[cy - 3:cy + 4, cx - 3:cx + 4]
            gxs, gys, d = gx[w].ravel(), gy[w].ravel(), dif[w].ravel()
            rows.append([np.sum(gxs * gxs, dtype=F32), np.sum(gxs * gys, dtype=F32), np.sum(gys * gys, dtype=F32),
                         np.sum(d * gxs, dtype=F32), np.sum(d * gys, dtype=F32)])
    return np.asarray(rows, F32)


def special_sums():
    tiny, den, inf = F32(1.1754944e-38), F32(1e-42), F32(np.inf)
    vals = [F32(0.0), F32(-0.0), den, -den, tiny, -tiny, inf, -inf, F32(1.0), F32(-3.5), F32(3.4e38), F32(1e-20)]
    rng = np.random.default_rng(22)
    rows = [rng.choice(vals, 5) for _ in range(4096)]
    # det = s * s on both sides of min_det (0.1f * 0.1f rounds just above 0.01f), with and without gxy
    s0 = F32(0.1)
    for k in range(-8, 9):
        s = s0
        for _ in range(abs(k)):
            s = np.nextafter(s, F32(1.0) if k > 0 else F32(0.0), dtype=F32)
        rows.append([s, F32(0.0), s, F32(0.3), F32(-0.2)])
        rows.append([s, F32(1e-3), s, F32(-7.0), F32(0.5)])
        rows.append([s * F32(100.0), F32(0.0), s / F32(100.0), F32(1e-3), F32(2.0)])
    return np.asarray(rows, F32)


def cases():
    rng = np.random.default_rng(21)
    rand = rng.integers(0, 2 ** 32, (2 ** 16, 5), dtype=np.uint32).view(F32)
    # random signs, exponents and mantissas near the tracker's range as well: most raw patterns give det = inf or NaN
    near = (rng.standard_normal((2 ** 14, 5)) * 10.0 ** rng.integers(-4, 7, (2 ** 14, 5))).astype(F32)
    near[:, 1] *= F32(0.1)
    return np.concatenate([scene_sums(), rand, near, special_sums()])


def solve_both(gpu, sums, step):
    from kltamd.device import check
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    n = len(sums)
    out, ok = np.full((n, 6), 7.0, F32), np.full(n, -1, np.int32)
    sums = np.ascontiguousarray(sums, F32)
    FP = C.POINTER(C.c_float)
    check(gpu, ctx, gpu.klt_hip_selftest_solve2(ctx, sums.ctypes.data_as(FP), step, float(MIN_DET),
                                                out.ctypes.data_as(FP), ok.ctypes.data_as(C.POINTER(C.c_int)), n),
          "selftest_solve2")
    gpu.KLTFreeTrackingContext(tc)
    return out.view(np.uint32), ok


@pytest.mark.parametrize("step", [1.0, 2.0])
def test_two_lanes_equal_the_uniform_solve(gpu, step):
    S = cases()
    with np.errstate(all="ignore"):
        det = S[:, 0] * S[:, 2] - S[:, 1] * S[:, 1]
    solved = ~(det < MIN_DET)  # a NaN det is not below min_det, as in the kernel
    n_scene = 13 * 251
    # the cases are what they are meant to be: both sides of min_det in the scene, the random and the special ones
    for part in (slice(0, n_scene), slice(n_scene, n_scene + 2 ** 16), slice(len(S) - 51, len(S))):
        assert 3 <= solved[part].sum() <= solved[part].size - 3, (part, solved[part].sum())
    assert np.isinf(S).any() and (S == 0).any() and ((np.abs(S) < 1.1754944e-38) & (S != 0)).any()
    out, ok = solve_both(gpu, S, step)
    assert np.array_equal(ok, np.where(solved, 7, 0)), "det < min_det: the variants or numpy disagree"
    for name, cols in (("from the sums' lanes", slice(2, 4)), ("from uniform sums", slice(4, 6))):
        bad = (out[:, cols] != out[:, 0:2]).any(axis=1)
        k = int(np.argmax(bad))
        assert not bad.any(), (f"two-lane solve {name}: {int(bad.sum())} of {len(S)} cases differ, first case {k}: "
                               f"sums {S[k].view(np.uint32)}, uniform {out[k, 0:2]}, two lanes {out[k, cols]}")
    assert (out[~solved] == 0).all()
    # and the uniform solve is the IEEE expression (numpy, one rounding per operation) where every
    # intermediate is zero or a normal number well inside the range
    with np.errstate(all="ignore"):
        ex, ey = S[:, 3] * F32(step), S[:, 4] * F32(step)
        p = [S[:, 0] * S[:, 2], S[:, 1] * S[:, 1], S[:, 2] * ex, S[:, 1] * ey, S[:, 0] * ey, S[:, 1] * ex]
        nx, ny = p[2] - p[3], p[4] - p[5]
        dx, dy = nx / det, ny / det
        mid = np.stack(p + [ex, ey, nx, ny, det, dx, dy])
        fin = solved & (((np.abs(mid) > 1e-30) & (np.abs(mid) < 1e30)) | (mid == 0)).all(axis=0)
    assert fin.sum() >= 2 ** 12, fin.sum()
    assert np.array_equal(out[fin, 0], dx[fin].view(np.uint32)) and np.array_equal(out[fin, 1], dy[fin].view(np.uint32))
