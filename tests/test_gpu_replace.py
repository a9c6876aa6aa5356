"""Lost features replaced inside the batched sequence calls
(klt_hip_set_frames_replace, KLTTrackSequenceReplace) and the trackability map
of an image-only level 0 (k_min_eigen7_img).

The definition is the loop

    track frame; if (count % every == 0) replace; store

so every case compares x, y, val, the aff_* fields and the table rows byte for
byte with that loop: run call by call on the same library, and run by the CPU
oracle.  Each case asserts its own condition (slots filled, a saturated frame,
nothing lost) from the oracle's run, so a case that stops being real fails.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import (AFF_RESET, GOLDEN, OracleTracker, affine_setup, arrays_to_fl, fl_affine, fl_to_arrays, parse_ft, u8ptr)
from test_gpu_multi import Dev

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, T = 160, 120, 13
FB_REJECTED = -6
IMG_KERNEL = b"k_min_eigen7_img"

_frames, _oracle = {}, {}


def same(a, b):
    """Byte for byte, every array of a against b's."""
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.shape == q.shape and p.dtype == q.dtype, i
        if p.tobytes() != q.tobytes():
            bad = np.argwhere(p.view(np.uint32) != q.view(np.uint32))
            raise AssertionError(f"array {i}: {len(bad)} differ, first {bad[:4].tolist()}: "
                                 f"{[p[tuple(j)] for j in bad[:4]]} != {[q[tuple(j)] for j in bad[:4]]}")


def frames_of(gpu, seed, w=W, h=H, n=T + 1):
    if (seed, w, h, n) not in _frames:
        _frames[seed, w, h, n] = [np.ascontiguousarray(f) for f in synth(gpu, seed, w, h, n)]
    return _frames[seed, w, h, n]


def oracle_loop(oracle, key, frames, n, every):
    """The loop on the CPU oracle from its own selection on frames[0]: the start
    list, the table [T, n] x 3, and per replacement point (frame, lost, filled)."""
    if (key, n, every) not in _oracle:
        o = OracleTracker(oracle)
        o.params.sequentialMode = 1
        oracle.orc_set_params(o.h, C.byref(o.params))
        x, y, v = o.select(frames[0], n)
        start = (x.copy(), y.copy(), v.copy())
        rows, points = [], []
        for i in range(1, len(frames)):
            o.track(frames[i - 1], frames[i], x, y, v)
            if i % every == 0:
                before = v.copy()
                if (before < 0).any():
                    o.replace(frames[i], x, y, v)
                points.append((i, int((before < 0).sum()), int(((before < 0) & (v >= 0)).sum())))
            rows.append((x.copy(), y.copy(), v.copy()))
        o.close()
        table = tuple(np.stack([r[k] for r in rows]) for k in range(3))
        _oracle[key, n, every] = (start, table, points)
    return _oracle[key, n, every]


def list_from(gpu, start):
    """A klt.h list holding `start` as a selection leaves it: KLTCreateFeatureList
    does not initialise the affine fields, _KLTSelectGoodFeatures does."""
    fl = gpu.KLTCreateFeatureList(len(start[0]))
    arrays_to_fl(fl, *start)
    for k in range(len(start[0])):
        f = fl.contents.feature[k].contents
        f.aff_x, f.aff_y, f.aff_Axx, f.aff_Ayx, f.aff_Axy, f.aff_Ayy = AFF_RESET
    return fl


def ft_arrays(ft, n, col0, ncol):
    cell = lambda j, i: ft.contents.feature[j][i].contents  # noqa: E731
    return tuple(np.array([[getattr(cell(j, col0 + i), f) for j in range(n)] for i in range(ncol)], dt)
                 for f, dt in (("x", F32), ("y", F32), ("val", np.int32)))


def run_klt(gpu, frames, start, every, batched, table=True, ft_col=0, setup=None, sequential=True, tail=None):
    """The loop call by call (batched False) or KLTTrackSequenceReplace (True) on
    a fresh tracking context, from the list `start`: the final list, its affine
    state and the table [T, n] x 3; the tracker kernel and the counters."""
    n, nt = len(start[0]), len(frames) - 1
    h, w = frames[0].shape
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1 if sequential else 0
    if setup:
        setup(tc.contents)
    fl = list_from(gpu, start)
    ft = gpu.KLTCreateFeatureTable(nt + ft_col, n) if table else None
    if batched:
        arr = (C.POINTER(C.c_ubyte) * len(frames))(*[u8ptr(f) for f in frames])
        gpu.KLTTrackSequenceReplace(tc, arr, len(frames), w, h, fl, ft, ft_col, every)
    else:
        for i in range(1, len(frames)):
            gpu.KLTTrackFeatures(tc, u8ptr(frames[i - 1]), u8ptr(frames[i]), w, h, fl)
            if i % every == 0:
                gpu.KLTReplaceLostFeatures(tc, u8ptr(frames[i]), w, h, fl)
            if ft:
                gpu.KLTStoreFeatureList(fl, ft, ft_col + i - 1)
    ctx = gpu.klt_amd_device_context(tc)
    kernel = gpu.klt_hip_track_kernel(ctx)
    on, fr, runs, filled = C.c_int(), C.c_long(), C.c_long(), C.c_long()
    assert gpu.klt_hip_get_frames_replace(ctx, C.byref(on), C.byref(fr), C.byref(runs), C.byref(filled)) == 0
    if tail:
        tail(tc, fl)
    out = fl_to_arrays(fl) + fl_affine(fl) + (ft_arrays(ft, n, ft_col, nt) if ft else ())
    gpu.KLTFreeFeatureList(fl)
    if ft:
        gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeTrackingContext(tc)
    return out, kernel, (on.value, fr.value, runs.value, filled.value)


def plain_kernel(gpu, frames, start):
    """The tracker kernel of a plain KLTTrackSequence of this shape."""
    n = len(start[0])
    h, w = frames[0].shape
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    fl = list_from(gpu, start)
    arr = (C.POINTER(C.c_ubyte) * len(frames))(*[u8ptr(f) for f in frames])
    gpu.KLTTrackSequence(tc, arr, len(frames), w, h, fl, None, 0)
    out = fl_to_arrays(fl)
    kernel = gpu.klt_hip_track_kernel(gpu.klt_amd_device_context(tc))
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    return kernel, out


# ---------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,border,skip", [(70, 40, 3, 0), (160, 120, 24, 0), (160, 120, 24, 1), (333, 251, 24, 0)])
def test_map_of_an_image_plane_equals_the_map_of_the_full_level(gpu, w, h, border, skip):
    from gpu_helpers import Dev as StageDev
    from kltamd.device import D2H, H2D, SelectDesc, check

    def setup(t):
        t.borderx = t.bordery = border
        t.nSkippedPixels = skip

    img = synth(gpu, 7000 + w, w, h, 1)[0]
    d = StageDev(gpu, setup)
    lib, ctx = gpu, d.ctx
    d.build(img, slot=0)
    assert d.path(0) == 1  # a fused slot
    want, nx, ny = d.eigen(0)
    assert b"k_min_eigen7<" in lib.klt_hip_eigen_kernel(ctx)
    assert nx * ny > 0
    plane = np.empty((h, w), F32)
    check(lib, ctx, lib.klt_hip_download_level(ctx, 0, 0, 0, plane.ctypes.data), "level")
    dimg = lib.klt_hip_malloc(ctx, plane.nbytes)
    dmap = lib.klt_hip_malloc(ctx, 4 * nx * ny)
    check(lib, ctx, lib.klt_hip_memcpy(ctx, dimg, plane.ctypes.data, plane.nbytes, H2D), "h2d")
    sd = SelectDesc(7, 7, border, border, skip)
    check(lib, ctx, lib.klt_hip_min_eigen_plane(ctx, dimg, w, h, C.byref(sd), dmap), "plane")
    assert IMG_KERNEL + (b"<%d>" % (skip + 1)) in lib.klt_hip_eigen_kernel(ctx)
    got = np.empty(nx * ny, np.int32)
    check(lib, ctx, lib.klt_hip_memcpy(ctx, got.ctypes.data, dmap, got.nbytes, D2H), "d2h")
    assert (want > 0).sum() > nx * ny // 2  # a map with content
    assert got.tobytes() == want.tobytes()
    for bad in (SelectDesc(9, 9, border + 1, border + 1, 0), SelectDesc(7, 7, border, border, 2)):
        assert lib.klt_hip_min_eigen_plane(ctx, dimg, w, h, C.byref(bad), dmap) == -1
        assert lib.klt_hip_last_error(ctx)
    lib.klt_hip_free(ctx, dimg)
    lib.klt_hip_free(ctx, dmap)
    d.close()


# ---------------------------------------------------------------------------
# 2. the reference's own REPLACE run
# ---------------------------------------------------------------------------
def test_reference_fixture(gpu, frames):
    seq = [np.ascontiguousarray(f) for f in [frames[1]] + list(frames[1:10])]
    h, w = seq[0].shape
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    fl = gpu.KLTCreateFeatureList(150)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(seq[0]), w, h, fl)
    ft = gpu.KLTCreateFeatureTable(10, 150)
    arr = (C.POINTER(C.c_ubyte) * len(seq))(*[u8ptr(f) for f in seq])
    gpu.KLTTrackSequenceReplace(tc, arr, len(seq), w, h, fl, ft, 0, 1)
    X, Y, V = ft_arrays(ft, 150, 0, 9)
    GX, GY, GV = parse_ft((GOLDEN / "seq_config1_replace_150x10.ft").read_bytes())
    for got, gold in ((X, GX), (Y, GY), (V, GV)):
        assert np.array_equal(got.T, gold[:, :9])
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeTrackingContext(tc)


# ---------------------------------------------------------------------------
# 3. against the per-call loop and the oracle's loop
# ---------------------------------------------------------------------------
def check_case(seed, n, every, start, points, table):
    """The condition that makes the case what it is, from the oracle's run."""
    if every == 64:
        assert not points
        return
    assert len(points) == T // every
    if (seed, n) == (160120, 60):
        assert all(filled > 0 for _, _, filled in points)
        if every == 3:
            assert [p[2] for p in points] == [7, 5, 5, 3]
    elif (seed, n) == (160120, 300):
        assert (start[2] < 0).sum() > 230  # the frame saturates: the selection itself finds no more
        assert all(1 <= filled <= 8 and lost > filled for _, lost, filled in points)  # the walk ends without filling all
        assert (table[2][-1] < 0).sum() > 230
    elif (seed, n) == (71, 40) and every == 1:
        assert [i for i, lost, _ in points if lost == 0] == [7, 8, 9, 10, 12, 13]  # the early-out
        assert any(filled > 0 for _, _, filled in points)


@pytest.mark.parametrize("every", [1, 3, 4, 5, 64])
@pytest.mark.parametrize("seed,n", [(160120, 60), (160120, 300), (71, 40)])
def test_equals_the_loop_and_the_oracle(gpu, oracle, seed, n, every):
    fr = frames_of(gpu, seed)
    start, table, points = oracle_loop(oracle, seed, fr, n, every)
    check_case(seed, n, every, start, points, table)
    want, _, _ = run_klt(gpu, fr, start, every, batched=False)
    got, kernel, (on, count, runs, filled) = run_klt(gpu, fr, start, every, batched=True)
    same(got, want)
    same(got[6:], table)  # the table rows are the oracle's
    want_kernel, plain = plain_kernel(gpu, fr, start)
    assert kernel == want_kernel and kernel.startswith(b"kltdev::k_track7")  # batched, not the fallback loop
    if every == 64:
        same(got[:3], plain)
        assert (on, count, runs, filled) == (0, 0, 0, 0)  # KLTTrackSequence itself: the setting was never on
    else:
        assert (on, count) == (0, T)  # off again, T frames counted
        assert runs == sum(1 for _, lost, _ in points if lost) and filled == sum(p[2] for p in points)


@pytest.mark.parametrize("table,ft_col", [(False, 0), (True, 2)])
def test_without_a_table_and_at_a_column(gpu, oracle, table, ft_col):
    fr = frames_of(gpu, 160120)
    start, otab, _ = oracle_loop(oracle, 160120, fr, 60, 3)
    want, _, _ = run_klt(gpu, fr, start, 3, batched=False, table=table, ft_col=ft_col)
    got, _, _ = run_klt(gpu, fr, start, 3, batched=True, table=table, ft_col=ft_col)
    same(got, want)
    assert np.array_equal(got[2], otab[2][-1]) and got[0].tobytes() == otab[0][-1].tobytes()
    if table:
        same(got[6:], otab)


# ---------------------------------------------------------------------------
# 4. the device call
# ---------------------------------------------------------------------------
def device_run(gpu, fr, start, every, chunk=4, calls=None, hook=None, budget=None, sd=None):
    """klt_hip_frames_begin on fr[0], then klt_hip_track_frames over the rest (in
    `calls` pieces) with the setting on: the table, the final list, the map
    kernel, the counters and the chunk used."""
    from kltamd.device import ReplaceDesc
    n, nt = len(start[0]), len(fr) - 1
    d = Dev(gpu, budget=budget)
    if hook:
        d.ok(getattr(gpu, hook[0])(d.ctx, hook[1]), hook[0])
    rd = ReplaceDesc.from_tc(d.tc.contents, every)
    d.ok(gpu.klt_hip_set_frames_replace(d.ctx, C.byref(rd)), "replace on")
    dfr = d.up(np.stack(fr))
    dx, dy, dv = d.up(start[0]), d.up(start[1]), d.up(start[2])
    tx, ty, tv = (d.up(np.zeros(nt * n, F32)) for _ in range(3))
    d.ok(gpu.klt_hip_frames_begin(d.ctx, C.byref(d.pd), dfr, W), "begin")
    j = 0
    for nf in calls or [nt]:
        off = 4 * j * n
        d.ok(gpu.klt_hip_track_frames(d.ctx, C.byref(d.pd), C.byref(d.td), dfr + (j + 1) * W * H, W, W * H, nf, chunk,
                                      dx, dy, dv, n, tx + off, ty + off, tv + off, n), "frames")
        j += nf
    assert j == nt
    out = (d.down(tx, (nt, n), F32), d.down(ty, (nt, n), F32), d.down(tv, (nt, n), np.int32),
           d.down(dx, n, F32), d.down(dy, n, F32), d.down(dv, n, np.int32))
    on, cnt, runs, filled = C.c_int(), C.c_long(), C.c_long(), C.c_long()
    d.ok(gpu.klt_hip_get_frames_replace(d.ctx, C.byref(on), C.byref(cnt), C.byref(runs), C.byref(filled)), "get")
    info = (gpu.klt_hip_eigen_kernel(d.ctx), (on.value, cnt.value, runs.value, filled.value),
            gpu.klt_hip_frames_chunk(d.ctx), d.kernel())
    d.close()
    return out, info


DEVICE_CASES = {
    "chunk1": dict(chunk=1), "chunk4": dict(chunk=4), "chunk64": dict(chunk=64),
    "split": dict(chunk=4, calls=[3, 4, 6]), "budget": dict(chunk=4, budget=2_000_000),
    "lazy_off": dict(hook=("klt_hip_set_lazy_grad", 0)), "merge_off": dict(hook=("klt_hip_set_track_merge", 0)),
    "prio_off": dict(hook=("klt_hip_set_track_prio", 0)), "input_order": dict(hook=("klt_hip_set_track_order", 1)),
    "overlap": dict(hook=("klt_hip_set_frames_overlap", 2)),
}


@pytest.mark.parametrize("case", sorted(DEVICE_CASES))
def test_device_call(gpu, oracle, case):
    fr = frames_of(gpu, 160120)
    start, table, points = oracle_loop(oracle, 160120, fr, 60, 3)
    assert [p[2] for p in points] == [7, 5, 5, 3]
    kw = DEVICE_CASES[case]
    out, (eig, counters, chunk, kernel) = device_run(gpu, fr, start, 3, **kw)
    same(out[:3], table)
    same(out[3:], tuple(t[-1] for t in table))
    assert counters == (1, T, 4, 20)
    if case == "budget":
        assert chunk == 2
    if case == "lazy_off":  # full records in the banks: the map kernel that reads gradients
        assert b"k_min_eigen7<1>" in eig and IMG_KERNEL not in eig
    else:
        assert IMG_KERNEL + b"<1>" in eig
        assert b"k_track7" in kernel


# ---------------------------------------------------------------------------
# 5. the processing order in play (n >= 2048)
# ---------------------------------------------------------------------------
def test_with_the_processing_order(gpu, oracle):
    fr = frames_of(gpu, 333, 333, 251)
    start, table, points = oracle_loop(oracle, "333x251", fr, 2100, 3)
    assert [p[2] for p in points] == [16, 9, 10, 13]
    assert 1650 < (table[2][-1] < 0).sum() < 1800
    got, kernel, (_, count, runs, filled) = run_klt(gpu, fr, start, 3, batched=True)
    same(got[6:], table)
    same(got[:3], tuple(t[-1] for t in table))
    assert (count, runs, filled) == (T, 4, 48) and kernel.startswith(b"kltdev::k_track7")


# ---------------------------------------------------------------------------
# 6. longer than the host pipeline's 16-frame chunk
# ---------------------------------------------------------------------------
def test_longer_than_a_host_chunk(gpu, oracle):
    fr = frames_of(gpu, 160120, n=21)
    start, table, points = oracle_loop(oracle, "21 frames", fr, 60, 5)
    assert len(points) == 4 and all(p[2] > 0 for p in points)
    want, _, _ = run_klt(gpu, fr, start, 5, batched=False)
    got, _, (_, count, runs, _) = run_klt(gpu, fr, start, 5, batched=True)
    same(got, want)
    same(got[6:], table)
    assert (count, runs) == (20, 4)


# ---------------------------------------------------------------------------
# 7. with the forward-backward check
# ---------------------------------------------------------------------------
def test_with_the_forward_backward_check(gpu, oracle, syn333):
    fr = [np.ascontiguousarray(f) for f in syn333]
    o = OracleTracker(oracle)
    start = o.select(fr[0], 300)
    o.close()

    def setup(t):
        assert gpu.klt_amd_set_fb_check(C.byref(t), 1, 0.05) == 0

    every = 2
    want, _, _ = run_klt(gpu, fr, start, every, batched=False, setup=setup)
    V = want[8]  # [frames, n]
    refilled = [(k, j) for j in range(V.shape[0] - 1) for k in np.nonzero(V[j] == FB_REJECTED)[0]
                if (V[j + 1:, k] >= 0).any()]
    assert refilled  # a slot the check rejected, refilled by a later replacement
    got, kernel, (_, count, runs, _) = run_klt(gpu, fr, start, every, batched=True, setup=setup)
    same(got, want)
    assert b"_fb" in kernel and count == 7 and runs >= 1


# ---------------------------------------------------------------------------
# 8. fallbacks equal the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["not_sequential", "affine"])
def test_fallbacks_equal_the_loop(gpu, oracle, which):
    fr = frames_of(gpu, 160120)[:8]
    start, _, _ = oracle_loop(oracle, 160120, frames_of(gpu, 160120), 60, 3)
    kw = dict(sequential=False) if which == "not_sequential" else dict(setup=affine_setup(mode=1))
    want, _, _ = run_klt(gpu, fr, start, 3, batched=False, **kw)
    got, _, (on, count, _, _) = run_klt(gpu, fr, start, 3, batched=True, **kw)
    same(got, want)
    assert (on, count) == (0, 0)  # the loop itself: the setting was never on
    assert (want[2] >= 0).sum() > 30
    if which == "affine":
        assert want[4].sum() > 10  # stored windows


# ---------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu, oracle):
    from kltamd.device import AffineDesc, ReplaceDesc, SelectDesc
    fr = frames_of(gpu, 160120)
    start, _, _ = oracle_loop(oracle, 160120, fr, 60, 3)
    n = 60
    d = Dev(gpu)
    ctx = d.ctx
    good = ReplaceDesc.from_tc(d.tc.contents, 3)
    on = C.c_int(7)
    for bad in (ReplaceDesc(good.sel, 10, 1, 0), ReplaceDesc(SelectDesc(7, 7, 2, 24, 0), 10, 1, 3),
                ReplaceDesc(SelectDesc(7, 7, 24, 24, -1), 10, 1, 3)):
        assert gpu.klt_hip_set_frames_replace(ctx, C.byref(bad)) == -1 and d.error()
        d.ok(gpu.klt_hip_get_frames_replace(ctx, C.byref(on), None, None, None), "get")
        assert on.value == 0
    d.ok(gpu.klt_hip_set_frames_replace(ctx, C.byref(good)), "on")
    dfr = d.up(np.stack(fr))
    dx, dy, dv = d.up(start[0]), d.up(start[1]), d.up(start[2])
    esc = d.up(np.zeros(1, np.int32))
    d.ok(gpu.klt_hip_frames_begin(ctx, C.byref(d.pd), dfr, W), "begin")
    pd, td = C.byref(d.pd), C.byref(d.td)
    cur = C.c_int(0)
    n_seq = (C.c_int * 1)(n)

    def untouched(rc, word):
        assert rc == -1 and word in d.error(), d.error()
        assert gpu.klt_hip_track_kernel(ctx) == b""  # no tracker launch so far
        same((d.down(dx, n, F32), d.down(dy, n, F32), d.down(dv, n, np.int32)), start)

    untouched(gpu.klt_hip_track_frames_band(ctx, pd, td, dfr + W * H, W, W * H, 4, dx, dy, dv, n, -np.inf, np.inf, 0, H,
                                            esc, None, 0), b"track_frames_band")
    untouched(gpu.klt_hip_track_frames_multi(ctx, pd, td, dfr, W, W * H, (T + 1) * W * H, 1, 4, 4, n_seq, dx, dy, dv,
                                             None, None, None, n), b"track_frames_multi")
    untouched(gpu.klt_hip_track_sequence(ctx, pd, td, dfr, W, W * H, 1, 4, dx, dy, dv, n, C.byref(cur)),
              b"track_sequence")
    affine_setup(mode=1)(d.tc.contents)
    ad = AffineDesc.from_tc(d.tc.contents)
    aff, state = d.up(np.zeros(6 * n, F32)), d.up(np.zeros(n, np.int32))
    assert gpu.klt_hip_affine_reserve(ctx, n, 15, 15) >= 0
    d.ok(gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), aff, state), "affine on")
    untouched(gpu.klt_hip_track_frames(ctx, pd, td, dfr + W * H, W, W * H, 4, 4, dx, dy, dv, n, None, None, None, 0),
              b"affine")
    d.ok(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "affine off")
    # and with the affine check off again the same call tracks
    d.ok(gpu.klt_hip_track_frames(ctx, pd, td, dfr + W * H, W, W * H, 4, 4, dx, dy, dv, n, None, None, None, 0), "frames")
    assert gpu.klt_hip_track_kernel(ctx).startswith(b"kltdev::k_track7")
    d.ok(gpu.klt_hip_ctx_reset(ctx), "reset")
    d.ok(gpu.klt_hip_get_frames_replace(ctx, C.byref(on), None, None, None), "get")
    assert on.value == 0 and gpu.klt_hip_eigen_kernel(ctx) == b""  # reset turns it off
    d.close()


# ---------------------------------------------------------------------------
# 10. afterwards
# ---------------------------------------------------------------------------
def test_per_call_tracking_continues_afterwards(gpu, oracle):
    all_fr = frames_of(gpu, 160120)
    start, _, _ = oracle_loop(oracle, 160120, all_fr, 60, 3)
    fr, a, b = all_fr[:11], all_fr[10], all_fr[11]

    def tail(tc, fl):
        gpu.KLTTrackFeatures(tc, u8ptr(a), u8ptr(b), W, H, fl)
        gpu.KLTReplaceLostFeatures(tc, u8ptr(b), W, H, fl)

    want, _, _ = run_klt(gpu, fr, start, 3, batched=False, tail=tail)
    got, _, _ = run_klt(gpu, fr, start, 3, batched=True, tail=tail)
    same(got, want)
    assert (want[2] >= 0).sum() > 40
