"""The processing order's balanced layout on the device (k_band_order).

klt_hip_band_order_probe runs the kernel as a whole-frame tracker launch
would; its order must be a permutation, keep the live features' bands
non-decreasing through the segments, and put live features into exactly the
slots klt_hip_order_slot names (tests/test_order_host.py holds that function
to the formula).  One end-to-end case tracks the same list in three orders --
balanced, lost-last (KLT_ORDER_BALANCE=0, read once per process, so in a child
process) and input order -- and compares lists and table rows byte for byte.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

F32 = np.float32
NS = [1, 4, 37, 2048, 2051, 5000, 20000]
XCDS, WAVES, BANDS, NROWS = 8, 4, 128, 480
W, H, T, CHUNK, N, SEED = 640, 480, 7, 4, 2304, 640480


def xcd_per_of(n):
    return ((n + WAVES - 1) // WAVES + XCDS - 1) // XCDS


def band_of(y):
    """k_band_order's band of a live feature, in float as the kernel computes it"""
    b = y.astype(F32) * (F32(BANDS) / F32(NROWS))
    with np.errstate(invalid="ignore"):
        return np.where(b >= 0, np.where(b < BANDS, np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64),
                                         BANDS - 1), 0)


def ys_of(kind, n, rng):
    if kind == "random":
        return rng.uniform(0, NROWS, n).astype(F32)
    if kind == "constant":
        return np.full(n, 123.25, F32)
    if kind == "nan":
        y = rng.uniform(0, NROWS, n).astype(F32)
        y[::2] = np.nan
        return y
    y = rng.uniform(-3 * NROWS, 4 * NROWS, n).astype(F32)  # out of range on both sides
    y[::5] = np.inf
    y[1::5] = -np.inf
    return y


def probe(gpu, ctx, y, v):
    from kltamd.device import H2D, check
    n = len(y)
    dy, dv = gpu.klt_hip_malloc(ctx, 4 * n), gpu.klt_hip_malloc(ctx, 4 * n)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dy, y.ctypes.data, y.nbytes, H2D), "h2d")
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dv, v.ctypes.data, v.nbytes, H2D), "h2d")
    perm = np.full(n, -9, np.int32)
    check(gpu, ctx, gpu.klt_hip_band_order_probe(ctx, dy, dv, n, NROWS, perm.ctypes.data), "probe")
    gpu.klt_hip_free(ctx, dy)
    gpu.klt_hip_free(ctx, dv)
    return perm


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "constant", "nan", "outside"])
@pytest.mark.parametrize("n", NS)
def test_probe_order(gpu, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    y = ys_of(kind, n, rng)
    v = np.zeros(n, np.int32)
    v[rng.permutation(n)[:n // 3]] = -1  # a third lost
    v[v == 0] = rng.integers(0, 3, int((v == 0).sum()))  # live values are >= 0
    tc = gpu.KLTCreateTrackingContext()
    perm = probe(gpu, gpu.klt_amd_device_context(tc), y, v)
    gpu.KLTFreeTrackingContext(tc)
    assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation"
    live_slot = v[perm] >= 0
    n_live = int((v >= 0).sum())
    # the live slots are the host function's
    want = np.zeros(n, bool)
    s = C.c_int()
    for r in range(n_live):
        assert gpu.klt_hip_order_slot(n, xcd_per_of(n), n_live, r, 0, C.byref(s)) == 0
        want[s.value] = True
    S = WAVES * xcd_per_of(n)
    seg = np.arange(n) // S
    assert np.array_equal(np.bincount(seg[live_slot], minlength=XCDS), np.bincount(seg[want], minlength=XCDS))
    assert np.array_equal(live_slot, want)
    # live features in slot order: bands never decrease, through every segment
    assert (np.diff(band_of(y[perm[live_slot]])) >= 0).all()


def start_list():
    """2304 hand-placed features: every third preset lost, every seventh close
    enough to the border to go out of bounds in the first frames"""
    rng = np.random.default_rng(N)
    x = rng.uniform(40, W - 40, N).astype(F32)
    y = rng.uniform(40, H - 40, N).astype(F32)
    v = np.zeros(N, np.int32)
    v[::3] = -1
    x[1::7] = rng.uniform(4.0, 9.0, len(x[1::7])).astype(F32)
    return x, y, v


def track(lib, frames, lazy, input_order):
    """frames[0] -> frames[1..T] in chunks of CHUNK: the table rows and the final list"""
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check
    x, y, v = start_list()
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = lib.klt_amd_device_context(tc)
    assert lib.klt_hip_set_lazy_grad(ctx, lazy) == 0
    assert lib.klt_hip_set_track_order(ctx, input_order) == 0
    stack = np.ascontiguousarray(np.stack(frames[:T + 1]))
    dfr = lib.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * N) for _ in range(3))
    tx, ty, tv = (lib.klt_hip_malloc(ctx, 4 * N * T) for _ in range(3))
    check(lib, ctx, lib.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    for d, a in ((dx, x), (dy, y), (dv, v)):
        check(lib, ctx, lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))
    check(lib, ctx, lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
    check(lib, ctx, lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + W * H, W, W * H, T, CHUNK, dx, dy,
                                             dv, N, tx, ty, tv, N), "frames")
    check(lib, ctx, lib.klt_hip_sync(ctx), "sync")
    X, Y, V = np.empty((T, N), F32), np.empty((T, N), F32), np.empty((T, N), np.int32)
    for d, a in ((tx, X), (ty, Y), (tv, V), (dx, x), (dy, y), (dv, v)):
        check(lib, ctx, lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
    for d in (dfr, dx, dy, dv, tx, ty, tv):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    return dict(X=X, Y=Y, V=V, x=x, y=y, v=v)


@pytest.fixture(scope="module")
def lost_last(tmp_path_factory):
    """both paths tracked lost-last, in one child process"""
    out = tmp_path_factory.mktemp("order") / "lost_last.npz"
    env = dict(os.environ, KLT_ORDER_BALANCE="0")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", [1, 0])
def test_three_orders_give_the_same_bytes(gpu, syn640, lost_last, lazy):
    assert os.environ.get("KLT_ORDER_BALANCE", "1") != "0"  # this process is the balanced one
    bal = track(gpu, syn640, lazy, 0)
    V = bal["V"]
    assert (V[-1] == 0).sum() > 300  # the case is real: features survive,
    assert ((V[0] < 0) & (start_list()[2] >= 0)).sum() > 100  # and some die in the first frames
    inp = track(gpu, syn640, lazy, 1)
    for k, a in bal.items():
        assert a.tobytes() == inp[k].tobytes(), ("input order", k)
        assert a.tobytes() == lost_last[f"{k}{lazy}"].tobytes(), ("lost last", k)


if __name__ == "__main__":  # the child: KLT_ORDER_BALANCE=0 is set in its environment
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import kltamd
    from conftest import synth
    assert os.environ.get("KLT_ORDER_BALANCE") == "0"
    lib_ = kltamd.load()
    lib_.KLTSetVerbosity(0)
    frames_ = synth(lib_, SEED, W, H, T + 1)
    res = {}
    for lazy_ in (1, 0):
        res.update({f"{k}{lazy_}": a for k, a in track(lib_, frames_, lazy_, 0).items()})
    np.savez(sys.argv[1], **res)
