"""Level-0 gradients computed by the tracker (klt_hip_set_lazy_grad).

With the switch on (the default) a plain batched call keeps level 0 of its
pyramid banks as the image plane alone and k_track7's lazy-gradient instances
compute gx / gy of the pixels their windows read.  Every case here compares
bit for bit: with the oracle where the oracle covers the call, else with the
same sequence run with the switch off (full level-0 records, the old path).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import OracleTracker
from test_gpu_track import _edge_positions, assert_table_equal, batch_sequence, batch_sequence_opts

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_switch(gpu, frames, nfeat, chunks, on, calls=None, setup=None, counts=None):
    """batch_sequence with klt_hip_set_lazy_grad(on) set before the first call."""
    def hook(ctx, done=False):
        if not done:
            assert gpu.klt_hip_set_lazy_grad(ctx, on) == 0
    return batch_sequence(gpu, frames, nfeat, chunks, setup=setup, calls=calls, counts=counts, ctx_hook=hook)


@pytest.fixture(scope="module")
def seq640(gpu, oracle):
    frames = synth(gpu, 5150, 640, 480, 12)
    return frames, OracleTracker(oracle).harness(frames, 1000, 12, first=frames[0])


@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("chunks,calls", [([1], None), ([5], None), ([64], None), ([2, 7], [3, 8])])
def test_switch_on_and_off_vs_oracle(gpu, seq640, chunks, calls, on):
    """Both switch positions equal the oracle, so they equal each other; with
    the default on, this keeps the full-record path covered."""
    frames, want = seq640
    X, Y, V = run_switch(gpu, frames, 1000, chunks, on, calls=calls)
    assert_table_equal(X, Y, V, *want)


def test_default_is_on_and_reset_restores_it(gpu):
    """The tracker kernel of a plain batched call is the lazy-gradient
    instance by default, the full-record one with the switch off; a context
    parked with the switch off comes back with the default (klt_hip_ctx_reset)."""
    frames = synth(gpu, 5150, 640, 480, 3)
    names = {}
    for on in (0, None, 1):
        def hook(ctx, done=False, on=on):
            if not done and on is not None:
                assert gpu.klt_hip_set_lazy_grad(ctx, on) == 0
            if done:
                names[on] = gpu.klt_hip_track_kernel(ctx).decode()
        batch_sequence(gpu, frames, 200, [2], ctx_hook=hook)
    lazy = "kltdev::k_track7<false, true, 2, false, true>"
    assert names[None] == lazy and names[1] == lazy, names
    assert names[0] == "kltdev::k_track7<false, true, 2, false>", names


def test_odd_size(gpu, oracle):
    """333x251: edge tiles on every side, a width that is no multiple of 64 or 4."""
    frames = synth(gpu, 333, 333, 251, 9)
    X, Y, V = run_switch(gpu, frames, 300, [3], 1)
    assert_table_equal(X, Y, V, *OracleTracker(oracle).harness(frames, 300, 9, first=frames[0]))


def test_one_level(gpu, oracle):
    """nPyramidLevels = 1 (the fused path allows it): level 0 is the coarsest
    level too, so the deferred residue rides with a lazy first pass."""
    from kltabi import OracleParams
    frames = synth(gpu, 334, 333, 251, 6)

    def setup(t):
        t.nPyramidLevels = 1

    X, Y, V = run_switch(gpu, frames, 200, [4], 1, setup=setup)
    tc = gpu.KLTCreateTrackingContext()
    setup(tc.contents)
    p = OracleParams.from_tc(tc.contents)
    gpu.KLTFreeTrackingContext(tc)
    assert_table_equal(X, Y, V, *OracleTracker(oracle, p).harness(frames, 200, 6, first=frames[0]))


def _largest_in(n):
    """The largest float x that passes the window bounds test for a dimension
    n: not ((float)n - (x + 3) < 1.001f), in float arithmetic."""
    lo, hi = F32(3.0).view(np.int32), F32(n).view(np.int32)
    ok = lambda b: not (F32(n) - (np.int32(b).view(F32) + F32(3.0)) < F32(1.001))
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return np.int32(lo).view(F32)


def _border_positions(w, h):
    """x and y from {3.0, 3.5, just below 6.0, the largest float that passes the
    bounds test, that minus 2.5} in every combination (both levels' limits: a
    level-1 coordinate is a quarter of these), plus mid-frame partners so that
    every border value also meets an ordinary one, plus _edge_positions()."""
    def axis(n):
        top = _largest_in(n)
        return [F32(3.0), F32(3.5), np.nextafter(F32(6.0), F32(0)), top, top - F32(2.5)]
    ax, ay = axis(w), axis(h)
    xs, ys = [], []
    for x in ax + [F32(w / 2 + 0.25)]:
        for y in ay + [F32(h / 2 + 0.75)]:
            xs.append(x)
            ys.append(y)
    # level-1 limits: level-0 positions whose quarter is at the level-1 bounds
    for x in (F32(12.0), F32(4.0) * _largest_in(w // 4)):
        for y in (F32(12.0), F32(4.0) * _largest_in(h // 4), F32(h / 2)):
            xs.append(x)
            ys.append(y)
    ex, ey = _edge_positions()
    return np.concatenate([np.array(xs, F32), ex]), np.concatenate([np.array(ys, F32), ey])


def _track_from(gpu, frames, x0, y0, on, chunk, setup):
    """klt_hip_frames_begin on frames[0], then one klt_hip_track_frames call over
    frames[1:] from the given positions; the table [T, n]."""
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check
    h, w = frames[0].shape
    n, T = len(x0), len(frames) - 1
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    setup(tc.contents)
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_set_lazy_grad(ctx, on) == 0
    stack = np.ascontiguousarray(np.stack(frames))
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv = (gpu.klt_hip_malloc(ctx, 4 * n) for _ in range(3))
    tx, ty, tv = (gpu.klt_hip_malloc(ctx, 4 * n * T) for _ in range(3))
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    for d, a in ((dx, x0.astype(F32)), (dy, y0.astype(F32)), (dv, np.zeros(n, np.int32))):
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, T, chunk,
                                             dx, dy, dv, n, tx, ty, tv, n), "frames")
    X, Y, V = np.empty((T, n), F32), np.empty((T, n), F32), np.empty((T, n), np.int32)
    for d, a in ((tx, X), (ty, Y), (tv, V)):
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
    for d in (dfr, dx, dy, dv, tx, ty, tv):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
    return X, Y, V


@pytest.mark.parametrize("nlev,chunk", [(2, 3), (1, 3), (1, 1)])
def test_hand_placed_border_features(gpu, oracle, nlev, chunk):
    """Features at the limits of the window bounds test at both levels, in all
    border and corner combinations, and at the cell-crossing positions: where
    the zero-border rule and the clamped patch loads decide the gradients.
    The context's border is 3, so that a feature there is kept, not declared
    out of bounds after the track.  With two levels a feature must pass level
    1's bounds first (level-0 position >= 12); with one level the level-0
    limits decide.  chunk 1: every launch is one frame, its image 1 the whole
    pyramid of the seed slot (first) or the previous launch's image-only bank
    frame."""
    from kltabi import OracleParams
    frames = synth(gpu, 778, 640, 480, 4)
    x0, y0 = _border_positions(640, 480)
    n = len(x0)

    def setup(t):
        t.nPyramidLevels = nlev
        t.borderx = t.bordery = 3

    tc = gpu.KLTCreateTrackingContext()
    setup(tc.contents)
    p = OracleParams.from_tc(tc.contents)
    gpu.KLTFreeTrackingContext(tc)
    ot = OracleTracker(oracle, p)
    ot.params.sequentialMode = 1
    oracle.orc_set_params(ot.h, C.byref(ot.params))
    ox, oy, ov = x0.copy(), y0.copy(), np.zeros(n, np.int32)
    OX, OY, OV = (np.zeros((n, 3), t) for t in (F32, F32, np.int32))
    for t in range(1, 4):
        ot.track(frames[t - 1], frames[t], ox, oy, ov)
        OX[:, t - 1], OY[:, t - 1], OV[:, t - 1] = ox, oy, ov
    print(f"\nhand-placed, {nlev} level(s): {int((OV[:, 0] == 0).sum())} of {n} tracked by the oracle")
    assert (OV[:, 0] == 0).any()  # the case is real: some of these track
    for on in (1, 0):
        X, Y, V = _track_from(gpu, frames, x0, y0, on, chunk, setup)
        assert_table_equal(X, Y, V, OX, OY, OV)


def test_overlapped_schedule_1080p(gpu, oracle):
    """Two streams, chunk 3 over 10 frames, 1080p, 5000 features, switch on."""
    frames = synth(gpu, 1080, 1920, 1080, 11)
    orig = gpu.klt_amd_device_context

    def hooked(tc):
        ctx = orig(tc)
        assert gpu.klt_hip_set_lazy_grad(ctx, 1) == 0
        return ctx

    gpu.klt_amd_device_context = hooked
    try:
        X, Y, V = batch_sequence_opts(gpu, frames, 5000, 3, dict(overlap=1))
    finally:
        gpu.klt_amd_device_context = orig
    assert_table_equal(X, Y, V, *OracleTracker(oracle).harness(frames, 5000, 11, first=frames[0]))


def test_work_counters(gpu, oracle, seq640):
    """klt_hip_set_track_count keeps its meaning with the switch on: systems
    formed equal the oracle's Newton loop bodies, gather round trips at least
    one per system."""
    frames, _ = seq640
    counts = []
    X, Y, V = run_switch(gpu, frames, 1000, [5], 1, counts=counts)
    oracle.orc_solve_count(1)
    want = OracleTracker(oracle).harness(frames, 1000, 12, first=frames[0])
    assert_table_equal(X, Y, V, *want)
    solves, passes = counts
    assert solves == oracle.orc_solve_count(1) and solves > 0
    assert passes >= solves


# ---------------------------------------------------------------------------
# readers of the kept pyramid after an image-only call
# ---------------------------------------------------------------------------
def _mixed_calls(gpu, frames, nfeat, on, second):
    """A plain klt_hip_track_frames call over frames[1:5] with the switch as
    given, then `second` over frames[5:]: "fb" (a call with the forward-
    backward check on), "band" (a whole-frame band call), "plain_off" (a plain
    call with the switch off).  Returns the lists after each call."""
    from kltabi import fl_to_arrays, u8ptr
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check
    h, w = frames[0].shape
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = gpu.klt_amd_device_context(tc)
    fl = gpu.KLTCreateFeatureList(nfeat)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(frames[0])), w, h, fl)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    stack = np.ascontiguousarray(np.stack(frames))
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv = (gpu.klt_hip_malloc(ctx, 4 * nfeat) for _ in range(3))
    esc = gpu.klt_hip_malloc(ctx, 4)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, esc, np.zeros(1, np.int32).ctypes.data, 4, H2D), "h2d")
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    for d, a in ((dx, x), (dy, y), (dv, v)):
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    out = []

    def grab():
        for d, a in ((dx, x), (dy, y), (dv, v)):
            check(gpu, ctx, gpu.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        out.append((x.copy(), y.copy(), v.copy()))

    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    assert gpu.klt_hip_set_lazy_grad(ctx, on) == 0
    check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, 4, 3, dx, dy, dv,
                                             nfeat, None, None, None, 0), "frames")
    grab()
    rest, nrest = dfr + 5 * w * h, len(frames) - 5
    if second == "fb":
        check(gpu, ctx, gpu.klt_hip_set_fb(ctx, 1, 0.5), "fb on")
        check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), rest, w, w * h, nrest, 2, dx, dy, dv,
                                                 nfeat, None, None, None, 0), "fb frames")
        check(gpu, ctx, gpu.klt_hip_set_fb(ctx, 0, 0.0), "fb off")
    elif second == "band":
        check(gpu, ctx, gpu.klt_hip_track_frames_band(ctx, C.byref(pd), C.byref(td), rest, w, w * h, nrest, dx, dy, dv,
                                                      nfeat, 0.0, float(h), 0, h, esc, None, 0), "band frames")
    else:
        assert gpu.klt_hip_set_lazy_grad(ctx, 0) == 0
        check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), rest, w, w * h, nrest, 2, dx, dy, dv,
                                                 nfeat, None, None, None, 0), "plain frames")
    grab()
    e = np.zeros(1, np.int32)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, e.ctypes.data, esc, 4, D2H), "d2h")
    assert e[0] == 0
    for d in (dfr, dx, dy, dv, esc):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
    return out


@pytest.mark.parametrize("second", ["fb", "band", "plain_off"])
def test_call_in_another_layout_follows(gpu, seq640, second):
    """A call that needs level-0 gradients of the kept pyramid (forward-
    backward, band, switch off) after an image-only call: the kept frame is
    made whole first.  Equal to the same calls with the switch off throughout;
    without the forward-backward check, to the oracle as well."""
    frames, want = seq640
    frames = frames[:9]
    a = _mixed_calls(gpu, frames, 1000, 1, second)
    b = _mixed_calls(gpu, frames, 1000, 0, second)
    for (xa, ya, va), (xb, yb, vb) in zip(a, b):
        assert np.array_equal(va, vb)
        assert np.array_equal(xa.view(np.int32), xb.view(np.int32))
        assert np.array_equal(ya.view(np.int32), yb.view(np.int32))
    assert (a[1][2] == 0).sum() > 100
    if second != "fb":
        OX, OY, OV = want
        for k, col in ((0, 3), (1, 7)):
            assert np.array_equal(a[k][2], OV[:, col])
            assert np.array_equal(a[k][0].view(np.int32), OX[:, col].view(np.int32))
            assert np.array_equal(a[k][1].view(np.int32), OY[:, col].view(np.int32))


def test_bank_reallocation_over_image_only_kept_frame(gpu, seq640):
    """A lazy call of 4 frames at chunk 2, then one of 4 frames at chunk 4 on
    the same, fresh context: the second call finds its banks too small while
    the kept pyramid is an image-only frame of one of them, so that frame is
    made whole in the seed slot and the banks are laid out again.  Equal, bit
    for bit, to the 8 frames tracked by a fresh context in one call.  The
    footprints show that the context came without banks and ends with banks
    of 4 frames (three banks, 3 floats per level-0 pixel)."""
    frames = seq640[0][:9]
    h, w = frames[0].shape
    foot = []

    def hook(ctx, done=False):
        foot.append(gpu.klt_hip_ctx_footprint(ctx))

    gpu.klt_amd_release_cached_devices()
    got = batch_sequence(gpu, frames, 256, [2, 4], calls=[4, 4], ctx_hook=hook)
    assert foot[0] < 3 * 2 * w * h * 12 and foot[1] - foot[0] >= 3 * 4 * w * h * 12
    gpu.klt_amd_release_cached_devices()
    want = batch_sequence(gpu, frames, 256, [8])
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert (got[2][-1] == 0).sum() > 25


def test_track_and_replace_after_sequence(gpu, oracle):
    """KLTTrackSequence (image-only banks), then per-call KLTTrackFeatures and
    KLTReplaceLostFeatures -- the tracker and the selection map read the kept
    pyramid's level-0 gradients -- against the oracle's per-frame loop."""
    from kltabi import fl_to_arrays, u8ptr
    frames = synth(gpu, 6162, 333, 251, 9)
    h, w = frames[0].shape
    n = 300
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(frames[0]), w, h, fl)
    keep = [np.ascontiguousarray(f) for f in frames[:6]]
    arr = (C.POINTER(C.c_ubyte) * 6)(*[u8ptr(f) for f in keep])
    gpu.KLTTrackSequence(tc, arr, 6, w, h, fl, None, 0)
    gpu.KLTReplaceLostFeatures(tc, u8ptr(frames[5]), w, h, fl)  # sequential mode: the kept pyramid's gradients
    got = [fl_to_arrays(fl)]
    for t in range(6, 9):
        gpu.KLTTrackFeatures(tc, u8ptr(np.zeros_like(frames[0])), u8ptr(frames[t]), w, h, fl)
        gpu.KLTReplaceLostFeatures(tc, u8ptr(frames[t]), w, h, fl)
        got.append(fl_to_arrays(fl))
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    ot = OracleTracker(oracle)
    ot.params.sequentialMode = 1
    oracle.orc_set_params(ot.h, C.byref(ot.params))
    x, y, v = ot.select(frames[0], n)
    for t in range(1, 6):
        ot.track(frames[t - 1], frames[t], x, y, v)
    ot.replace(frames[5], x, y, v)
    want = [(x.copy(), y.copy(), v.copy())]
    for t in range(6, 9):
        ot.track(frames[t - 1], frames[t], x, y, v)
        ot.replace(frames[t], x, y, v)
        want.append((x.copy(), y.copy(), v.copy()))
    for (gx, gy, gv), (wx, wy, wv) in zip(got, want):
        assert np.array_equal(gv, wv)
        assert np.array_equal(gx.view(np.int32), wx.view(np.int32))
        assert np.array_equal(gy.view(np.int32), wy.view(np.int32))


def test_level_getters_after_image_only_call(gpu):
    """klt_hip_frames_end_slot after an image-only call, then the level
    getters: every plane of every level equals a full build of that frame."""
    from kltamd.device import H2D, PyrDesc, TrackDesc, check
    frames = synth(gpu, 335, 333, 251, 4)
    h, w = frames[0].shape
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_set_lazy_grad(ctx, 1) == 0
    stack = np.ascontiguousarray(np.stack(frames))
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, 3, 2, None, None,
                                             None, 0, None, None, None, 0), "frames")
    check(gpu, ctx, gpu.klt_hip_frames_end_slot(ctx, 0), "end_slot")
    check(gpu, ctx, gpu.klt_hip_build_pyramid(ctx, 1, C.byref(pd), dfr + 3 * w * h, w, 1), "build")
    for lvl in range(tc.contents.nPyramidLevels):
        lw, lh = C.c_int(0), C.c_int(0)
        check(gpu, ctx, gpu.klt_hip_level_dims(ctx, 0, lvl, C.byref(lw), C.byref(lh)), "dims")
        assert gpu.klt_hip_level_interleaved(ctx, 0, lvl) == gpu.klt_hip_level_interleaved(ctx, 1, lvl)
        for which in range(3):
            a = np.full((lh.value, lw.value), -7.0, F32)
            b = np.full((lh.value, lw.value), -9.0, F32)
            check(gpu, ctx, gpu.klt_hip_download_level(ctx, 0, lvl, which, a.ctypes.data), "download")
            check(gpu, ctx, gpu.klt_hip_download_level(ctx, 1, lvl, which, b.ctypes.data), "download")
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (lvl, which)
    gpu.klt_hip_free(ctx, dfr)
    gpu.KLTFreeTrackingContext(tc)


def test_fast_reduction_with_switch_on(gpu):
    """KLT_HIP_FAST sums on image-only banks stay within
    test_fast_reduction_tolerance's own bounds on its own sequence (config 2)."""
    from test_gpu_long import (FAST_MAX_DRIFT_PX, FAST_MAX_FLIP_FRACTION, device_run, fast_vs_exact, first_mismatch,
                               fixture)
    cfg = fixture("config2")
    Xe, Ye, Ve = device_run(gpu, cfg)  # exact sums, switch on by default
    assert first_mismatch(Xe, Ye, Ve, cfg["columns"]) is None
    Xf, Yf, Vf = device_run(gpu, cfg, reduction=1)
    st = fast_vs_exact(Xe, Ye, Ve, Xf, Yf, Vf)
    print(f"\nfast reduction, lazy gradients: {st}")
    assert st["flip_fraction"] <= FAST_MAX_FLIP_FRACTION, st
    assert st["max_dx"] <= FAST_MAX_DRIFT_PX and st["max_dy"] <= FAST_MAX_DRIFT_PX, st
    assert st["tracked_in_both"] > 0.5 * st["cells"]
