"""Forward-backward (FB) consistency check on the GPU (klt_hip_set_fb,
klt_amd_set_fb_check) against the oracle composition of tests/test_fb.py:
bit patterns of x and y, exact val, exact e, on every path that honours FB."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import KLTRunner, OracleParams, arrays_to_fl, fl_to_arrays, u8ptr
from test_fb import (FB_REJECTED, OracleStepper, assert_splits, bits, fb_compose, fb_counts, load_fb_fixture)
from test_gpu_track import assert_table_equal, batch_sequence

pytestmark = pytest.mark.gpu

# the oracle's result for a case, computed once and shared (never modified)
_WANT: dict = {}


def want(oracle, key, frames, n, max_dist, params=None, replace=False, nframes=None, start=None):
    if key not in _WANT:
        st = {}
        r = fb_compose(OracleStepper(oracle, params), frames, n, nframes or len(frames), max_dist, first=frames[0],
                       replace=replace, stats=st, start=start)
        for a in r:
            a.setflags(write=False)
        _WANT[key] = r + (st["rejected"],)
    return _WANT[key]


def fb_setup(gpu, max_dist, more=None):
    """tc_setup callback: FB on for the tracking context behind `t`."""
    def setup(t):
        if more:
            more(t)
        assert gpu.klt_amd_set_fb_check(C.byref(t), 1, max_dist) == 0
    return setup


def params_of(gpu, setup):
    tc = gpu.KLTCreateTrackingContext()
    setup(tc.contents)
    p = OracleParams.from_tc(tc.contents)
    gpu.KLTFreeTrackingContext(tc)
    return p


def assert_cols_equal(got, exp, ncols):
    """[n, frames] tables (the harness's layout) over the written columns."""
    for g, w, name in zip(got, exp, "xyv"):
        assert np.array_equal(bits(g[:, :ncols]), bits(w[:, :ncols])), name


class ErrTable:
    """The optional FB-error table on a device context, one row per frame."""

    def __init__(self, gpu, ctx, rows, n):
        from kltamd.device import check
        self.gpu, self.ctx, self.rows, self.n = gpu, ctx, rows, n
        self.buf = gpu.klt_hip_malloc(ctx, 4 * rows * n)
        fill = np.full((rows, n), 7.0, np.float32)  # every cell must be written
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, self.buf, fill.ctypes.data, fill.nbytes, 1), "h2d")

    def point(self, row):
        assert self.gpu.klt_hip_set_fb_table(self.ctx, self.buf + 4 * row * self.n, self.n) == 0

    def take(self):
        from kltamd.device import D2H, check
        E = np.empty((self.rows, self.n), np.float32)
        check(self.gpu, self.ctx, self.gpu.klt_hip_sync(self.ctx), "sync")
        check(self.gpu, self.ctx, self.gpu.klt_hip_memcpy(self.ctx, E.ctypes.data, self.buf, E.nbytes, D2H), "d2h")
        assert self.gpu.klt_hip_set_fb_table(self.ctx, None, 0) == 0
        self.gpu.klt_hip_free(self.ctx, self.buf)
        return E


# ---------------------------------------------------------------------------
# 1. single KLTTrackFeatures calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sequential", [True, False])
@pytest.mark.parametrize("max_dist", [0.02, 0.05, 1.0])
def test_single_calls(gpu, oracle, frames, max_dist, sequential):
    OX, OY, OV, OE, _ = want(oracle, ("img", max_dist), frames, 100, max_dist)
    if max_dist == 0.05:
        assert_splits(OV)
    assert fb_counts(OV)[0] == {0.02: 81, 0.05: 23, 1.0: 0}[max_dist]
    tab = {}

    def setup(t):
        fb_setup(gpu, max_dist)(t)
        ctx = gpu.klt_amd_device_context(C.byref(t))
        tab["t"] = ErrTable(gpu, ctx, 1, 100)
        tab["t"].point(0)

    rows = []

    def on_frame(i, fl):  # row 0 holds this call's distances
        from kltamd.device import D2H, check
        t = tab["t"]
        e = np.empty(100, np.float32)
        check(gpu, t.ctx, gpu.klt_hip_memcpy(t.ctx, e.ctypes.data, t.buf, e.nbytes, D2H), "d2h")
        rows.append(e)
        if i == 9:
            t.take()

    got = KLTRunner(gpu).harness(frames, 100, 10, first=frames[0], sequential=sequential, tc_setup=setup,
                                 on_frame=on_frame)
    assert_cols_equal(got, (OX, OY, OV), 9)
    assert np.array_equal(bits(np.stack(rows)), bits(OE))
    if max_dist == 0.05:
        d, FX, FY, FV, FE = load_fb_fixture()
        assert_cols_equal(got, (FX, FY, FV), 9)
        assert np.array_equal(bits(np.stack(rows)), bits(FE))


# ---------------------------------------------------------------------------
# 2.-4. the batched path (klt_hip_track_frames)
# ---------------------------------------------------------------------------
def batch_fb(gpu, frames, nfeat, chunks, max_dist, calls=None, setup=None, hooks=None, start=None):
    """test_gpu_track.batch_sequence with FB on and the error table pointed at
    each call's first row; hooks: tuning setters applied to the context.
    Returns X, Y, V ([T, n]) and E ([T, n])."""
    T = len(frames) - 1
    state = {"row": 0}
    orig = gpu.klt_hip_track_frames

    def call(ctx, *args):
        if "tab" not in state:
            assert gpu.klt_hip_set_fb(ctx, 1, max_dist) == 0
            for name, val in (hooks or {}).items():
                assert getattr(gpu, name)(ctx, val) == 0, name
            state["tab"] = ErrTable(gpu, ctx, T, nfeat)
        state["tab"].point(state["row"])
        state["row"] += args[5]  # nframes of this call
        return orig(ctx, *args)

    def hook(ctx, done=False):
        if done:
            state["E"] = state["tab"].take()

    gpu.klt_hip_track_frames = call
    try:
        X, Y, V = batch_sequence(gpu, frames, nfeat, chunks, setup, calls=calls, ctx_hook=hook, start=start)
    finally:
        gpu.klt_hip_track_frames = orig
    return X, Y, V, state["E"]


def assert_batch_equal(got, exp):
    X, Y, V, E = got
    OX, OY, OV, OE = exp[:4]
    assert_table_equal(X, Y, V, OX, OY, OV)
    assert np.array_equal(bits(E), bits(OE[:E.shape[0]])), "e differs"


@pytest.mark.parametrize("max_dist", [0.05, 0.02, 1.0])
@pytest.mark.parametrize("chunks,calls", [([1], None), ([3], None), ([7], None), ([2, 7], [3, 4])])
def test_batched_vs_oracle(gpu, oracle, syn333, chunks, calls, max_dist):
    """Chunk and call boundaries: the backward pass of a chunk's first frame
    reads the previous bank's (or the seed's) pyramid as its image 2."""
    exp = want(oracle, ("syn333", max_dist), syn333, 300, max_dist)
    if max_dist == 0.05:
        assert_splits(exp[2])
        assert fb_counts(exp[2]) == (19, 267)
    elif max_dist == 0.02:
        assert fb_counts(exp[2])[0] == 64
    else:  # nothing comes back farther than a pixel: every rejection is a lost backward pass
        assert fb_counts(exp[2])[0] == 7 and ((exp[2] == FB_REJECTED).T[:7] <= (exp[3] < 0)).all()
    assert_batch_equal(batch_fb(gpu, syn333, 300, chunks, max_dist, calls=calls), exp)


def test_generic_kernel_window9(gpu, oracle):
    frames = synth(gpu, 98, 333, 251, 8)

    def setup(t):
        t.window_width = t.window_height = 9
        gpu.KLTUpdateTCBorder(C.byref(t))  # the border that goes with the window

    exp = want(oracle, "w9", frames, 200, 0.05, params_of(gpu, setup))
    assert_splits(exp[2])
    assert_batch_equal(batch_fb(gpu, frames, 200, [3], 0.05, setup=setup), exp)


def test_generic_kernel_lighting_insensitive(gpu, oracle, syn333):
    def setup(t):
        t.lighting_insensitive = 1

    exp = want(oracle, "li", syn333, 300, 0.05, params_of(gpu, setup))
    assert_splits(exp[2])
    assert_batch_equal(batch_fb(gpu, syn333, 300, [3], 0.05, setup=setup), exp)


def test_generic_kernel_equals_default_kernel(gpu, oracle, syn333):
    """klt_hip_set_track_impl(ctx, 1): the generic kernel's FB instance at the
    default configuration."""
    exp = want(oracle, ("syn333", 0.05), syn333, 300, 0.05)
    assert_batch_equal(batch_fb(gpu, syn333, 300, [3], 0.05, hooks=dict(klt_hip_set_track_impl=1)), exp)


@pytest.mark.parametrize("hooks", [dict(klt_hip_set_track_order=1), dict(klt_hip_set_track_patch=0),
                                   dict(klt_hip_set_track_merge=0), dict(klt_hip_set_track_merge=1),
                                   dict(klt_hip_set_track_prio=0), dict(klt_hip_set_frames_overlap=1),
                                   dict(klt_hip_set_track_order=1, klt_hip_set_track_patch=0,
                                        klt_hip_set_frames_overlap=1)])
def test_tuning_hooks_do_not_change_fb_results(gpu, oracle, syn640, hooks):
    """2100 features: past the threshold from which the band order is sorted."""
    fr = syn640[:6]
    exp = want(oracle, "syn640", fr, 2100, 0.05)
    assert_splits(exp[2])
    assert_batch_equal(batch_fb(gpu, fr, 2100, [2], 0.05, hooks=hooks), exp)


# ---------------------------------------------------------------------------
# 5. KLTTrackSequence
# ---------------------------------------------------------------------------
def test_track_sequence_stays_batched(gpu, oracle, syn640):
    from kltamd.device import Timing, check
    fr = [np.ascontiguousarray(f) for f in syn640[:6]]
    n, T, (h, w) = 1000, 5, fr[0].shape
    OX, OY, OV, OE, _ = want(oracle, "syn640/1000", fr, n, 0.05)
    assert_splits(OV)
    loop = KLTRunner(gpu).harness(fr, n, 6, first=fr[0], tc_setup=fb_setup(gpu, 0.05))
    assert_cols_equal(loop, (OX, OY, OV), T)

    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    assert gpu.klt_amd_set_fb_check(tc, 1, 0.05) == 0
    ctx = gpu.klt_amd_device_context(tc)
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(fr[0]), w, h, fl)
    ft = gpu.KLTCreateFeatureTable(T, n)
    arr = (C.POINTER(C.c_ubyte) * len(fr))(*[u8ptr(f) for f in fr])
    tm = Timing()
    check(gpu, ctx, gpu.klt_hip_set_timing(ctx, 1), "timing on")
    check(gpu, ctx, gpu.klt_hip_get_timing(ctx, C.byref(tm)), "timing reset")
    gpu.KLTTrackSequence(tc, arr, len(fr), w, h, fl, ft, 0)
    check(gpu, ctx, gpu.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
    check(gpu, ctx, gpu.klt_hip_set_timing(ctx, 0), "timing off")
    assert tm.frames_track == T and 0 < tm.n_track < T  # fewer tracker launches than frames
    assert b"_fb" in gpu.klt_hip_track_kernel(ctx)
    cell = lambda j, i: ft.contents.feature[j][i].contents  # noqa: E731
    X = np.array([[cell(j, i).x for i in range(T)] for j in range(n)], np.float32)
    Y = np.array([[cell(j, i).y for i in range(T)] for j in range(n)], np.float32)
    V = np.array([[cell(j, i).val for i in range(T)] for j in range(n)], np.int32)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    assert_cols_equal((X, Y, V), (OX, OY, OV), T)
    assert np.array_equal(v, OV[:, T - 1]) and np.array_equal(bits(x), bits(OX[:, T - 1]))
    assert int((v >= 0).sum()) == fb_counts(OV)[1]


# ---------------------------------------------------------------------------
# 6. replacement
# ---------------------------------------------------------------------------
def test_replace_refills_rejected_slots(gpu, oracle, syn333):
    OX, OY, OV, OE, rejected = want(oracle, "syn333/replace", syn333[:4], 300, 0.05, replace=True)
    assert rejected >= 3 and (OV[:, :3] >= 0).all()  # rejected, and every slot refilled
    got = KLTRunner(gpu).harness(syn333[:4], 300, 4, first=syn333[0], replace=True, tc_setup=fb_setup(gpu, 0.05))
    assert_cols_equal(got, (OX, OY, OV), 3)


# ---------------------------------------------------------------------------
# 7. off again, and a fresh context
# ---------------------------------------------------------------------------
def test_fb_off_again_and_fresh_context(gpu, oracle, syn333):
    from kltabi import OracleTracker
    a, b = syn333[0], syn333[1]
    h, w = a.shape
    n = 300
    tc = gpu.KLTCreateTrackingContext()
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(a), w, h, fl)
    x0, y0, v0 = fl_to_arrays(fl)

    def track():
        arrays_to_fl(fl, x0, y0, v0)
        gpu.KLTTrackFeatures(tc, u8ptr(a), u8ptr(b), w, h, fl)
        return fl_to_arrays(fl)

    plain = track()
    assert gpu.klt_amd_set_fb_check(tc, 1, 0.05) == 0
    on = track()
    assert (on[2] == FB_REJECTED).sum() >= 3 and (plain[2] != FB_REJECTED).all()
    assert gpu.klt_amd_set_fb_check(tc, 0, 0.05) == 0
    off = track()
    ox, oy, ov = x0.copy(), y0.copy(), v0.copy()
    ot = OracleTracker(oracle)
    ot.params.sequentialMode = 0
    oracle.orc_set_params(ot.h, C.byref(ot.params))
    ot.track(a, b, ox, oy, ov)
    for g in (plain, off):
        assert np.array_equal(g[2], ov) and np.array_equal(bits(g[0]), bits(ox)) and np.array_equal(bits(g[1]),
                                                                                                     bits(oy))
    kept = on[2] >= 0  # a kept feature is exactly the forward result
    assert np.array_equal(bits(on[0][kept]), bits(ox[kept])) and np.array_equal(bits(on[1][kept]), bits(oy[kept]))

    # freed with FB on: the parked device context is handed out with FB off
    assert gpu.klt_amd_set_fb_check(tc, 1, 0.05) == 0
    track()
    ctx = gpu.klt_amd_device_context(tc)
    flag, dist = C.c_int(-1), C.c_float(-1.0)
    assert gpu.klt_hip_get_fb(ctx, C.byref(flag), C.byref(dist)) == 0
    assert flag.value == 1 and dist.value == np.float32(0.05)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_get_fb(ctx, C.byref(flag), C.byref(dist)) == 0
    assert flag.value == 0
    fl = gpu.KLTCreateFeatureList(n)
    fresh = track()
    assert np.array_equal(fresh[2], ov) and np.array_equal(bits(fresh[0]), bits(ox))
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)


# ---------------------------------------------------------------------------
# 8. what FB does not cover fails before any launch
# ---------------------------------------------------------------------------
def test_errors(gpu, syn333):
    from kltamd.device import FAST, H2D, PyrDesc, Timing, TrackDesc, check

    class AffineDesc(C.Structure):
        _fields_ = [("mode", C.c_int), ("window_width", C.c_int), ("window_height", C.c_int),
                    ("max_iterations", C.c_int), ("min_determinant", C.c_float), ("min_displacement", C.c_float),
                    ("affine_min_displacement", C.c_float), ("max_residue", C.c_float),
                    ("max_displacement_differ", C.c_float), ("step_factor", C.c_float),
                    ("lighting_insensitive", C.c_int)]

    h, w = syn333[0].shape
    n = 64
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert gpu.klt_hip_set_fb(ctx, 1, bad) < 0
        assert b"max_dist" in gpu.klt_hip_last_error(ctx)
    flag, dist = C.c_int(-1), C.c_float(-1.0)
    assert gpu.klt_hip_get_fb(ctx, C.byref(flag), C.byref(dist)) == 0 and flag.value == 0
    assert gpu.klt_hip_set_fb(ctx, 1, 0.05) == 0

    stack = np.ascontiguousarray(np.stack(syn333[:3]))
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv, esc = (gpu.klt_hip_malloc(ctx, 4 * n) for _ in range(4))
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    feat = np.zeros(n, np.float32) + 100.0
    for d in (dx, dy):
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, d, feat.ctypes.data, feat.nbytes, H2D), "h2d")
    zeros = np.zeros(n, np.int32)
    for d in (dv, esc):
        check(gpu, ctx, gpu.klt_hip_memcpy(ctx, d, zeros.ctypes.data, zeros.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    check(gpu, ctx, gpu.klt_hip_build_pyramid(ctx, 0, C.byref(pd), dfr, w, 0), "build 0")
    check(gpu, ctx, gpu.klt_hip_build_pyramid(ctx, 1, C.byref(pd), dfr + w * h, w, 0), "build 1")
    tm = Timing()
    check(gpu, ctx, gpu.klt_hip_set_timing(ctx, 1), "timing on")
    check(gpu, ctx, gpu.klt_hip_get_timing(ctx, C.byref(tm)), "timing reset")

    # the band call
    rc = gpu.klt_hip_track_frames_band(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, 2, dx, dy, dv, n,
                                       0.0, float(h), 0, h, esc, None, 0)
    assert rc < 0 and b"forward-backward" in gpu.klt_hip_last_error(ctx)
    # fast sums: batched, single call on device arrays, sequence
    fast = TrackDesc.from_buffer_copy(td)
    fast.reduction = FAST
    rc = gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(fast), dfr + w * h, w, w * h, 2, 2, dx, dy, dv, n,
                                  None, None, None, 0)
    assert rc < 0 and b"forward-backward" in gpu.klt_hip_last_error(ctx)
    rc = gpu.klt_hip_track(ctx, 0, 1, C.byref(fast), dx, dy, dv, n, 1)
    assert rc < 0 and b"forward-backward" in gpu.klt_hip_last_error(ctx)
    # the affine check
    ad = AffineDesc(2, 15, 15, 10, 0.01, 0.1, 0.02, 10.0, 1.5, 1.0, 0)
    fn = gpu.klt_hip_track_affine
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(TrackDesc), C.POINTER(AffineDesc)] + [C.c_void_p] * 5 + [
        C.c_int]
    hx, hy, hv, st = feat.copy(), feat.copy(), zeros.copy(), zeros.copy()
    aff = np.zeros(6 * n, np.float32)
    rc = fn(ctx, 0, 1, C.byref(td), C.byref(ad), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data, aff.ctypes.data,
            st.ctypes.data, n)
    assert rc < 0 and b"forward-backward" in gpu.klt_hip_last_error(ctx)
    assert np.array_equal(hx, feat) and np.array_equal(hv, zeros)

    check(gpu, ctx, gpu.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
    assert (tm.n_track, tm.n_pyr_l0, tm.n_pyr_l1, tm.n_generic) == (0, 0, 0, 0)  # nothing was launched
    got = np.empty(n, np.float32)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, got.ctypes.data, dx, got.nbytes, 2), "d2h")
    assert np.array_equal(got, feat)
    # an error table narrower than the list
    assert gpu.klt_hip_set_fb_table(ctx, esc, n - 1) == 0
    assert gpu.klt_hip_track(ctx, 0, 1, C.byref(td), dx, dy, dv, n, 1) < 0
    assert b"stride" in gpu.klt_hip_last_error(ctx)
    assert gpu.klt_hip_set_fb_table(ctx, None, 0) == 0
    # and with exact sums the same call goes through
    check(gpu, ctx, gpu.klt_hip_track(ctx, 0, 1, C.byref(td), dx, dy, dv, n, 1), "track")
    check(gpu, ctx, gpu.klt_hip_set_timing(ctx, 0), "timing off")
    for d in (dfr, dx, dy, dv, esc):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
