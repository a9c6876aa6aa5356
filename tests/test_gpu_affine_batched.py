"""The affine consistency check inside the batched tracker launch
(klt_hip_set_frames_affine, klt_hip_set_affine_table) on the GPU: every path
that honours the setting against the reference's fixtures and the oracle, on
bit patterns; the refusals; switching off."""
from __future__ import annotations

import ctypes as C
import sys
import zlib

import numpy as np
import pytest

from kltabi import (AFF_RESET, GOLDEN, OracleTracker, TrackingContextRec, affine_setup, fl_affine, fl_to_arrays,
                    u8ptr)
from test_gpu_track import assert_table_equal

sys.path.insert(0, str(GOLDEN))
from make_affine_batched import BATCHED_CASES  # noqa: E402
from make_golden import AFFINE_CASES, affine_inputs  # noqa: E402
from test_affine import FIELDS  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in AFFINE_CASES + BATCHED_CASES if not c[4]}  # replace cases have no batched form
AFF_KERNEL = "kltdev::k_track_frames_g_aff"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def golden(name):
    d = np.load(GOLDEN / f"{name}.npz")
    return tuple(d[k] for k in FIELDS)


def harness_seq(frames, nf):
    """The frames the kltabi harness feeds: selection on frames[1], then
    frames[1] .. frames[nf-1] tracked in turn (example3.c's loop)."""
    return [frames[1]] + list(frames[1:nf])


class Run:
    """What one device-resident run produced: X, Y, V, ST [T, n], AFF [T, n, 6]
    (the tables), the final list and arrays, per call the state array, the crc
    of every window held at the end, the tracker kernel's name."""


def run_device(gpu, seq, nfeat, setup, how="frames", chunks=(64,), calls=None, hooks=None, path=None,
               off=None):
    """Select on seq[0], track seq[1:] with the check inside the launch.
    how: "frames" klt_hip_track_frames (split into `calls`, one chunk size
    each), "host" klt_hip_track_frames_host, "sequence" klt_hip_track_sequence
    and "track" klt_hip_track(on_device=1), both one frame per call.
    off: "null" / "reset" turn the setting off again before tracking."""
    from kltamd.device import D2H, H2D, AffineDesc, PyrDesc, TrackDesc, check
    h, w = seq[0].shape
    T = len(seq) - 1
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    setup(tc.contents)
    ctx = gpu.klt_amd_device_context(tc)
    ck = lambda rc, what: check(gpu, ctx, rc, what)  # noqa: E731
    if path is not None:
        ck(gpu.klt_hip_set_path(ctx, path), "path")
    fl = gpu.KLTCreateFeatureList(nfeat)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(seq[0])), w, h, fl)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    ad = AffineDesc.from_tc(tc.contents)
    S3 = 3 * (ad.window_width + 2) * (ad.window_height + 2)
    stack = np.ascontiguousarray(np.stack(seq))
    aff = np.tile(np.array(AFF_RESET, np.float32), (nfeat, 1))
    state = np.zeros(nfeat, np.int32)
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv, ds = (gpu.klt_hip_malloc(ctx, 4 * nfeat) for _ in range(4))
    da = gpu.klt_hip_malloc(ctx, 4 * 6 * nfeat)
    tx, ty, tv, ts = (gpu.klt_hip_malloc(ctx, 4 * nfeat * T) for _ in range(4))
    ta = gpu.klt_hip_malloc(ctx, 4 * 6 * nfeat * T)
    fill = np.full(6 * nfeat * T, 7, np.int32)  # every table cell must be written
    for d, a in ((dfr, stack), (dx, x), (dy, y), (dv, v), (ds, state), (da, aff), (ta, fill), (ts, fill[:nfeat * T])):
        ck(gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    for name, val in (hooks or {}).items():
        ck(getattr(gpu, name)(ctx, val), name)
    assert gpu.klt_hip_affine_reserve(ctx, nfeat, ad.window_width, ad.window_height) >= 0
    ck(gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), da, ds), "set_frames_affine")
    on = C.c_int(-1)
    assert gpu.klt_hip_get_frames_affine(ctx, C.byref(on)) == 0 and on.value == 1
    if off == "null":
        ck(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "off")
    elif off == "reset":
        ck(gpu.klt_hip_ctx_reset(ctx), "reset")
    if off:
        assert gpu.klt_hip_get_frames_affine(ctx, C.byref(on)) == 0 and on.value == 0

    def point(row):  # the affine tables' row 0 for the next call
        if not off:
            ck(gpu.klt_hip_set_affine_table(ctx, ta + 4 * 6 * nfeat * row, ts + 4 * nfeat * row, nfeat), "table")

    def states():
        ck(gpu.klt_hip_sync(ctx), "sync")
        s = np.empty(nfeat, np.int32)
        ck(gpu.klt_hip_memcpy(ctx, s.ctypes.data, ds, s.nbytes, D2H), "d2h")
        return s

    r = Run()
    r.call_rows, r.call_states = [], []
    if how == "frames":
        ck(gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
        j0 = 0
        for nf, ch in zip(calls or [T], chunks):
            point(j0)
            o = 4 * nfeat * j0
            ck(gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + (1 + j0) * w * h, w, w * h, nf, ch, dx,
                                        dy, dv, nfeat, tx + o, ty + o, tv + o, nfeat), "track_frames")
            j0 += nf
            r.call_rows.append(j0 - 1)
            r.call_states.append(states())
        assert j0 == T
    elif how == "host":
        keep = [np.ascontiguousarray(f) for f in seq]
        arr = (C.POINTER(C.c_ubyte) * len(keep))(*[u8ptr(f) for f in keep])
        hx, hy, hv = x.copy(), y.copy(), v.copy()
        point(0)
        ck(gpu.klt_hip_track_frames_host(ctx, C.byref(pd), C.byref(td), arr, len(keep), 1, chunks[0],
                                         hx.ctypes.data, hy.ctypes.data, hv.ctypes.data, nfeat, None, None),
           "track_frames_host")
        for d, a in ((dx, hx), (dy, hy), (dv, hv)):
            ck(gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    else:
        ck(gpu.klt_hip_build_pyramid(ctx, 0, C.byref(pd), dfr, w, 0), "build")
        cur = C.c_int(0)
        for t in range(T):
            point(t)
            o = 4 * nfeat * t
            if how == "sequence":
                ck(gpu.klt_hip_track_sequence(ctx, C.byref(pd), C.byref(td), dfr, w, w * h, 1 + t, 1, dx, dy, dv,
                                              nfeat, C.byref(cur)), "track_sequence")
            else:
                nxt = (cur.value + 1) % 2
                ck(gpu.klt_hip_build_pyramid(ctx, nxt, C.byref(pd), dfr + (1 + t) * w * h, w, 0), "build")
                ck(gpu.klt_hip_track(ctx, cur.value, nxt, C.byref(td), dx, dy, dv, nfeat, 1), "track")
                cur.value = nxt
            for d, s in ((tx, dx), (ty, dy), (tv, dv)):  # these calls have no x / y / val table
                ck(gpu.klt_hip_memcpy(ctx, d + o, s, 4 * nfeat, 3), "d2d")
            r.call_rows.append(t)
            r.call_states.append(states())
    ck(gpu.klt_hip_sync(ctx), "sync")
    r.kernel = gpu.klt_hip_track_kernel(ctx).decode()
    r.X, r.Y = np.empty((T, nfeat), np.float32), np.empty((T, nfeat), np.float32)
    r.V, r.ST = np.empty((T, nfeat), np.int32), np.empty((T, nfeat), np.int32)
    r.AFF = np.empty((T, nfeat, 6), np.float32)
    r.aff, r.state = np.empty((nfeat, 6), np.float32), np.empty(nfeat, np.int32)
    for d, a in ((tx, r.X), (ty, r.Y), (tv, r.V), (ts, r.ST), (ta, r.AFF), (dx, x), (dy, y), (dv, v), (da, r.aff),
                 (ds, r.state)):
        ck(gpu.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
    r.x, r.y, r.v = x, y, v
    r.crc = np.zeros(nfeat, np.uint32)
    held = np.flatnonzero(r.state != 0).astype(np.int32)
    if len(held) and not off:
        win = np.empty((len(held), S3), np.float32)
        ck(gpu.klt_hip_affine_get(ctx, held.ctypes.data_as(C.POINTER(C.c_int)), len(held),
                                  win.ctypes.data_as(C.POINTER(C.c_float))), "affine_get")
        r.crc[held] = [zlib.crc32(wk.tobytes()) for wk in win]
    ck(gpu.klt_hip_set_affine_table(ctx, None, None, 0), "table off")
    ck(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "off")
    for d in (dfr, dx, dy, dv, ds, da, tx, ty, tv, ts, ta):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
    return r


def assert_run(r, want, tables=True):
    """r against X, Y, V [n, frames], AFF [T, n, 6], HAS, CRC [T, n] in the
    harness's layout (kltabi.run_affine)."""
    X, Y, V, A, H, K = want
    T = A.shape[0]
    assert r.kernel.startswith(AFF_KERNEL), r.kernel
    if tables:
        assert_table_equal(r.X, r.Y, r.V, X[:, :T], Y[:, :T], V[:, :T])
    assert np.array_equal(bits(r.AFF), bits(A))
    assert np.array_equal((r.ST != 0).astype(np.int32), H)
    assert set(np.unique(r.ST)) <= {0, 1, 2}
    assert np.array_equal(r.v, V[:, T - 1]) and np.array_equal(bits(r.x), bits(X[:, T - 1]))
    assert np.array_equal(bits(r.y), bits(Y[:, T - 1]))
    assert np.array_equal(bits(r.aff), bits(A[-1])) and np.array_equal(r.state, r.ST[-1])
    assert np.array_equal(r.crc, K[-1])
    # state 2 exactly for the windows stored in that call and still held
    before = np.zeros(H.shape[1], np.int32)
    for row, s in zip(r.call_rows, r.call_states):
        exp = np.where(H[row] == 0, 0, np.where(before == 1, 1, 2))
        assert np.array_equal(s, exp), f"states after the call ending at frame {row + 1}"
        before = H[row]


def case_setup(name):
    return affine_setup(**CASES[name][5])


def case_seq(name):
    _, data, n, nf, _, _ = CASES[name]
    return harness_seq(affine_inputs(data), nf), n


# ---------------------------------------------------------------------------
# fixtures, device-resident
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunks,calls", [([1], None), ([4], None), ([64], None), ([2, 7], [3, 6])])
@pytest.mark.parametrize("name", list(CASES))
def test_fixture_track_frames(gpu, name, chunks, calls):
    seq, n = case_seq(name)
    if calls and sum(calls) != len(seq) - 1:  # the 8-frame warp cases: 3 + 4 frames
        calls = [3, len(seq) - 1 - 3]
    assert_run(run_device(gpu, seq, n, case_setup(name), chunks=chunks, calls=calls), golden(name))


def test_cases_cover_every_non_replace_fixture():
    assert len(CASES) == len(AFFINE_CASES) - 1 + len(BATCHED_CASES) == 12


# ---------------------------------------------------------------------------
# pyramid paths
# ---------------------------------------------------------------------------
def test_generic_pyramid_path(gpu):
    """klt_hip_set_path(ctx, 1): generic kernels, banks of planes."""
    name = "affine_m2_w11_100x10"
    seq, n = case_seq(name)
    assert_run(run_device(gpu, seq, n, case_setup(name), chunks=[4], path=1), golden(name))


_ORACLE: dict = {}


def oracle_want(oracle, key, frames, n, nf, setup):
    """The oracle's run of a case, computed once and shared (never modified)."""
    if key not in _ORACLE:
        tc = TrackingContextRec()
        setup(tc)
        o = OracleTracker(oracle)
        o.params.lighting_insensitive = tc.lighting_insensitive
        res = o.harness_affine(frames, n, nf, tc)
        for a in res:
            a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def test_fused_pyramid_path(gpu, oracle, syn333):
    """333x251: the fused pyramid kernels on a size that is no multiple of a
    tile, interleaved banks turned into planes for the tracker."""
    from kltamd.device import PyrDesc
    setup = affine_setup(mode=2, window=9, max_it=6, min_disp=0.05)
    tc = gpu.KLTCreateTrackingContext()
    pd = PyrDesc()
    gpu.klt_amd_pyr_desc(tc, 333, 251, tc.contents.nPyramidLevels, 1, C.byref(pd))
    assert gpu.klt_hip_fused_path(gpu.klt_amd_device_context(tc), C.byref(pd)) == 1
    gpu.KLTFreeTrackingContext(tc)
    want = oracle_want(oracle, "syn333", syn333, 300, 8, setup)
    assert want[4][-1].sum() >= 20
    assert_run(run_device(gpu, harness_seq(syn333, 8), 300, setup, chunks=[3]), want)


# ---------------------------------------------------------------------------
# synthetic against the oracle
# ---------------------------------------------------------------------------
SYN_SETUP = affine_setup(mode=2, window=9, mdd=2.5)


def syn_want(oracle, syn640):
    return oracle_want(oracle, "syn640", syn640, 1000, 12, SYN_SETUP)


@pytest.mark.parametrize("hooks", [None, {"klt_hip_set_track_order": 1, "klt_hip_set_frames_overlap": 1}])
def test_synthetic_vs_oracle(gpu, oracle, syn640, hooks):
    want = syn_want(oracle, syn640)
    assert want[4][-1].sum() >= 20 and ((want[4][:-1] == 1) & (want[4][1:] == 0)).any()
    assert_run(run_device(gpu, harness_seq(syn640, 12), 1000, SYN_SETUP, chunks=[5], hooks=hooks), want)


# ---------------------------------------------------------------------------
# other entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["sequence", "track"])
def test_frame_by_frame_entry_points(gpu, how):
    name = "affine_m2_100x10"
    seq, n = case_seq(name)
    assert_run(run_device(gpu, seq, n, case_setup(name), how=how), golden(name))


def test_track_sequence_several_steps_per_call(gpu):
    """klt_hip_track_sequence over all frames in one call: a window stored in
    an early step is still state 2 at the end of the call."""
    from kltamd.device import D2H, H2D, AffineDesc, PyrDesc, TrackDesc, check
    name = "affine_m1_100x10"
    seq, n = case_seq(name)
    X, Y, V, A, H, K = golden(name)
    h, w = seq[0].shape
    T = len(seq) - 1
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    case_setup(name)(tc.contents)
    ctx = gpu.klt_amd_device_context(tc)
    ck = lambda rc, what: check(gpu, ctx, rc, what)  # noqa: E731
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(seq[0])), w, h, fl)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    ad = AffineDesc.from_tc(tc.contents)
    stack = np.ascontiguousarray(np.stack(seq))
    aff = np.tile(np.array(AFF_RESET, np.float32), (n, 1))
    state = np.zeros(n, np.int32)
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv, ds = (gpu.klt_hip_malloc(ctx, 4 * n) for _ in range(4))
    da = gpu.klt_hip_malloc(ctx, 4 * 6 * n)
    for d, a in ((dfr, stack), (dx, x), (dy, y), (dv, v), (ds, state), (da, aff)):
        ck(gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    assert gpu.klt_hip_affine_reserve(ctx, n, ad.window_width, ad.window_height) >= 0
    ck(gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), da, ds), "on")
    ck(gpu.klt_hip_build_pyramid(ctx, 0, C.byref(pd), dfr, w, 0), "build")
    cur = C.c_int(0)
    ck(gpu.klt_hip_track_sequence(ctx, C.byref(pd), C.byref(td), dfr, w, w * h, 1, T, dx, dy, dv, n, C.byref(cur)),
       "track_sequence")
    ck(gpu.klt_hip_sync(ctx), "sync")
    for d, a in ((dx, x), (dy, y), (dv, v), (ds, state), (da, aff)):
        ck(gpu.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
    ck(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "off")
    for d in (dfr, dx, dy, dv, ds, da):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
    assert np.array_equal(v, V[:, T - 1]) and np.array_equal(bits(x), bits(X[:, T - 1]))
    assert np.array_equal(bits(aff), bits(A[-1]))
    assert np.array_equal(state, 2 * H[-1])  # every held window was stored in this call


def test_track_frames_host(gpu):
    name = "affine_m2_w11_100x10"
    seq, n = case_seq(name)
    r = run_device(gpu, seq, n, case_setup(name), how="host", chunks=[4])
    r.call_rows, r.call_states = [len(seq) - 2], [r.state]
    assert_run(r, golden(name), tables=False)


def seq_api(gpu, seq, nfeat, setup, split=None):
    """KLTTrackSequence over seq with a feature table; split: hand the list to
    a fresh tracking context before frame `split` (its windows then live in
    aff_img only).  Returns the table's X, Y, V [n, T] and the final list."""
    h, w = seq[0].shape
    T = len(seq) - 1
    keep = [np.ascontiguousarray(f) for f in seq]

    def new_tc():
        tc = gpu.KLTCreateTrackingContext()
        tc.contents.sequentialMode = 1
        setup(tc.contents)
        return tc

    tc = new_tc()
    fl = gpu.KLTCreateFeatureList(nfeat)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(keep[0]), w, h, fl)
    ft = gpu.KLTCreateFeatureTable(T, nfeat)
    parts = [(0, len(keep))] if split is None else [(0, split), (split - 1, len(keep))]
    for k, (a, b) in enumerate(parts):
        if k:
            gpu.KLTFreeTrackingContext(tc)
            tc = new_tc()
        arr = (C.POINTER(C.c_ubyte) * (b - a))(*[u8ptr(f) for f in keep[a:b]])
        gpu.KLTTrackSequence(tc, arr, b - a, w, h, fl, ft, a)
    cell = lambda j, i: ft.contents.feature[j][i].contents  # noqa: E731
    X = np.array([[cell(j, i).x for i in range(T)] for j in range(nfeat)], np.float32)
    Y = np.array([[cell(j, i).y for i in range(T)] for j in range(nfeat)], np.float32)
    V = np.array([[cell(j, i).val for i in range(T)] for j in range(nfeat)], np.int32)
    last = fl_to_arrays(fl) + fl_affine(fl)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    return X, Y, V, last


@pytest.mark.parametrize("split", [None, 5])
def test_klt_track_sequence(gpu, split):
    """KLTTrackSequence with the check on == the KLTTrackFeatures +
    KLTStoreFeatureList loop (the reference's fixture) in every column and in
    the final list's affine state and window crcs; with `split`, the windows
    are uploaded from aff_img into a fresh context mid-sequence and the run
    continues as the uninterrupted one."""
    name = "affine_m2_100x10"
    seq, n = case_seq(name)
    WX, WY, WV, A, H, K = golden(name)
    T = len(seq) - 1
    X, Y, V, (x, y, v, aff, has, crc) = seq_api(gpu, seq, n, case_setup(name), split)
    assert np.array_equal(V, WV[:, :T]) and np.array_equal(bits(X), bits(WX[:, :T]))
    assert np.array_equal(bits(Y), bits(WY[:, :T]))
    assert np.array_equal(v, WV[:, T - 1]) and np.array_equal(bits(x), bits(WX[:, T - 1]))
    assert np.array_equal(bits(aff), bits(A[-1]))
    assert np.array_equal(has, H[-1]) and np.array_equal(crc, K[-1])
    assert has.sum() > 20


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu, frames):
    """Each call the setting does not cover returns -1 with a message before
    any launch and leaves the feature arrays untouched."""
    from kltamd.device import D2H, FAST, H2D, AffineDesc, PyrDesc, TrackDesc, check
    seq = harness_seq(frames, 4)
    h, w = seq[0].shape
    n = 50
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    affine_setup(mode=2)(tc.contents)
    ctx = gpu.klt_amd_device_context(tc)
    ck = lambda rc, what: check(gpu, ctx, rc, what)  # noqa: E731
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(seq[0])), w, h, fl)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    ad = AffineDesc.from_tc(tc.contents)
    stack = np.ascontiguousarray(np.stack(seq))
    aff = np.tile(np.array(AFF_RESET, np.float32), (n, 1))
    state = np.zeros(n, np.int32)
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv, ds, esc = (gpu.klt_hip_malloc(ctx, 4 * n) for _ in range(5))
    da, ta = (gpu.klt_hip_malloc(ctx, 4 * 6 * n) for _ in range(2))
    dev = ((dx, x), (dy, y), (dv, v), (ds, state), (da, aff))
    for d, a in ((dfr, stack),) + dev:
        ck(gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    for s in (0, 1):
        ck(gpu.klt_hip_build_pyramid(ctx, s, C.byref(pd), dfr + s * w * h, w, 0), "build")
    ck(gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")

    def frames_call(desc=td):
        return gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(desc), dfr + w * h, w, w * h, 3, 4, dx, dy, dv, n,
                                        None, None, None, 0)

    def refused(rc, word, c=ctx):
        assert rc == -1
        msg = gpu.klt_hip_last_error(c).decode()
        assert word in msg, msg
        ck(gpu.klt_hip_sync(ctx), "sync")
        for d, a in dev:
            got = np.empty_like(a)
            ck(gpu.klt_hip_memcpy(ctx, got.ctypes.data, d, a.nbytes, D2H), "d2h")
            assert np.array_equal(bits(got), bits(a)), word

    raw = gpu.klt_hip_ctx_create(-1)  # a context of its own: nothing reserved yet
    assert raw and gpu.klt_hip_frames_begin(raw, C.byref(pd), dfr, w) == 0
    assert gpu.klt_hip_set_frames_affine(raw, C.byref(ad), da, ds) == 0
    refused(gpu.klt_hip_track_frames(raw, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, 3, 4, dx, dy, dv, n,
                                     None, None, None, 0), "klt_hip_affine_reserve", raw)
    gpu.klt_hip_ctx_destroy(raw)
    assert gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), da, ds) == 0
    assert gpu.klt_hip_affine_reserve(ctx, n, 5, 5) >= 0
    refused(frames_call(), "klt_hip_affine_reserve")  # ... or for another window size
    assert gpu.klt_hip_affine_reserve(ctx, n, ad.window_width, ad.window_height) >= 0
    refused(gpu.klt_hip_track_frames_band(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, 3, dx, dy, dv, n,
                                          0.0, float(h), 0, h, esc, None, 0), "band")
    fast = TrackDesc.from_buffer_copy(td)
    fast.reduction = FAST
    refused(frames_call(fast), "KLT_HIP_EXACT")
    assert gpu.klt_hip_set_fb(ctx, 1, 0.05) == 0
    refused(frames_call(), "forward-backward")
    refused(gpu.klt_hip_track(ctx, 0, 1, C.byref(td), dx, dy, dv, n, 1), "forward-backward")
    assert gpu.klt_hip_set_fb(ctx, 0, 0.0) == 0
    hx, hy, hv = x.copy(), y.copy(), v.copy()
    refused(gpu.klt_hip_track(ctx, 0, 1, C.byref(td), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data, n, 0),
            "device arrays")
    ha, hs = aff.copy(), state.copy()
    F, I = C.POINTER(C.c_float), C.POINTER(C.c_int)
    refused(gpu.klt_hip_track_affine(ctx, 0, 1, C.byref(td), C.byref(ad), hx.ctypes.data_as(F),
                                     hy.ctypes.data_as(F), hv.ctypes.data_as(I), ha.ctypes.data_as(F),
                                     hs.ctypes.data_as(I), n), "klt_hip_set_frames_affine")
    for got, a in ((hx, x), (hy, y), (hv, v), (ha, aff), (hs, state)):
        assert np.array_equal(bits(got), bits(a))
    assert gpu.klt_hip_set_affine_table(ctx, ta, None, n - 1) == 0
    refused(frames_call(), "stride")
    assert gpu.klt_hip_set_affine_table(ctx, None, None, 0) == 0
    # bad descriptions leave the setting as it was
    bad = AffineDesc.from_buffer_copy(ad)
    bad.mode = 3
    assert gpu.klt_hip_set_frames_affine(ctx, C.byref(bad), da, ds) == -1
    bad.mode, bad.window_width = 2, 8
    assert gpu.klt_hip_set_frames_affine(ctx, C.byref(bad), da, ds) == -1
    assert gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), None, ds) == -1
    on = C.c_int(0)
    assert gpu.klt_hip_get_frames_affine(ctx, C.byref(on)) == 0 and on.value == 1
    ck(frames_call(), "the covered call still runs")
    assert gpu.klt_hip_track_kernel(ctx).decode().startswith(AFF_KERNEL)
    ck(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "off")
    ck(gpu.klt_hip_sync(ctx), "sync")
    for d in (dfr, dx, dy, dv, ds, esc, da, ta):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)


# ---------------------------------------------------------------------------
# switching off
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("off", ["null", "reset"])
def test_switching_off(gpu, oracle, frames, off):
    """After the setter with NULL, or klt_hip_ctx_reset, a run is the plain one."""
    seq = harness_seq(frames, 10)
    r = run_device(gpu, seq, 100, affine_setup(mode=2), chunks=[4], off=off)
    OX, OY, OV = OracleTracker(oracle).harness(frames, 100, 10)
    assert_table_equal(r.X, r.Y, r.V, OX, OY, OV)
    assert "aff" not in r.kernel
    assert (r.state == 0).all() and np.array_equal(bits(r.aff), bits(np.tile(np.array(AFF_RESET, np.float32), (100, 1))))
    assert (r.ST == 7).all()  # no table was written
