"""The kernel instance behind every public tracker and map call.

klt_hip_track_kernel / klt_hip_eigen_kernel report the instance the last launch
ran; callers (bench.py's matching of counter summaries, the tools) compare the
strings.  Each case below makes one call that the public API routes to one row
of the launchers' tables (csrc/track7.hip, track7_pred.hip, track7_mask.hip,
pyramid.hip) and asserts the name, written out here.  tests/test_kernel_names.py
holds every name to a kernel of its unit without a GPU; this file holds the
choice: settings -> row.

Scene: tests/motion_scenes.py's scene 7 (160x120), frames 0..2, every sixth of
the placed features (42).  Where the CPU oracle states the result the table and
the final list are compared to it by bit pattern: the exact-sum rows against
motion_scenes.oracle_placed (the mask rows too: an all-allowed mask loses
nothing), the forward-backward rows against test_gpu_fb.want, the motion-prior
rows in their first frame (a zero state is the plain tracker).  The fast-sum
rows are not bit-exact by design (tests/test_gpu_fast_sums.py holds them): the
name alone.

Settings that pick the row: interleaved levels or planes (klt_hip_set_path),
depth 2 or 1 (search range 2), the band call, klt_hip_set_fb, _set_predict,
_set_mask with KLT_HIP_MASK_TRACK, klt_hip_set_lazy_grad, the wave times
(klt_hip_set_wave_times) or the exit count (schedule 3 over two chunks), fast
sums (KLT_HIP_FAST), the multi-sequence call.

All 27 tracker rows and all 7 map rows are reached.  Two of them only in a
roundabout way, which is what the public API offers: band calls insist on the
fused pyramid path, so k_track7<true, false, 0, false> (band, planes) runs when
the kept pyramid was built as planes (klt_hip_frames_begin under
klt_hip_set_path 1) and the band call's bank is interleaved -- the launch then
reads both as planes; and k_min_eigen (the generic map kernel) needs a window
other than 7x7 or a step above 2.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import motion_scenes as ms
from test_gpu_fb import want as fb_want
from test_gpu_multi import Dev, H, W

pytestmark = pytest.mark.gpu

F32 = np.float32
NF = 3                        # frames 0..2: two tracked frames
PICK = slice(None, None, 6)   # 42 of the 251 placed features
MASK_TRACK = 2                # KLT_HIP_MASK_TRACK
FB_DIST = 0.05
K = "kltdev::"

# (expected name, settings)
TRACK_ROWS = [
    # lazy gradients (the batched call's default)
    (K + "k_track7<false, true, 2, false, true>", {}),
    (K + "k_track7<false, true, 0, false, true>", dict(one_level=1)),
    (K + "k_track7<false, true, 2, true, true>", dict(fast=1)),
    # ... with the wave times, or the exit count of the tail schedule
    (K + "k_track7_hook<2, false>", dict(times=1)),
    (K + "k_track7_hook<0, false>", dict(times=1, one_level=1)),
    (K + "k_track7_hook<2, true>", dict(times=1, fast=1)),
    (K + "k_track7_hook<2, false>", dict(exits=1)),
    # full level-0 records, planes, band calls: the names without the fifth argument
    (K + "k_track7<false, true, 2, false>", dict(lazy=0)),
    (K + "k_track7<false, true, 0, false>", dict(lazy=0, one_level=1)),
    (K + "k_track7<false, false, 0, false>", dict(planes=1)),
    (K + "k_track7<false, false, 0, false>", dict(planes=1, one_level=1)),
    (K + "k_track7<false, true, 2, true>", dict(lazy=0, fast=1)),
    (K + "k_track7<true, true, 2, false>", dict(band=1)),
    (K + "k_track7<true, true, 0, false>", dict(band=1, one_level=1)),
    (K + "k_track7<true, false, 0, false>", dict(band=1, planes_kept=1)),
    (K + "k_track7<true, true, 2, true>", dict(band=1, fast=1)),
    # the forward-backward check
    (K + "k_track7_fb<true, 2>", dict(fb=1)),
    (K + "k_track7_fb<true, 0>", dict(fb=1, one_level=1)),
    (K + "k_track7_fb<false, 0>", dict(fb=1, planes=1)),
    # the motion prior
    (K + "k_track7_pred<true, 2>", dict(pred=1)),
    (K + "k_track7_pred<true, 0>", dict(pred=1, one_level=1)),
    (K + "k_track7_pred<false, 0>", dict(pred=1, planes=1)),
    # the region mask's tracking use
    (K + "k_track7_mask_lazy<2>", dict(mask=1)),
    (K + "k_track7_mask_lazy<0>", dict(mask=1, one_level=1)),
    (K + "k_track7_mask<true, 2>", dict(mask=1, lazy=0)),
    (K + "k_track7_mask<true, 0>", dict(mask=1, lazy=0, one_level=1)),
    (K + "k_track7_mask<false, 0>", dict(mask=1, planes=1)),
]


def case_id(row):
    name, s = row
    return name[len(K):].replace(" ", "") + ("-" + "-".join(sorted(s)) if s else "")


def start_list():
    return tuple(np.ascontiguousarray(a[PICK]) for a in ms.placed_list())


def track(gpu, s):
    """One batched call (or band call) over frames 1..2 with settings s: the
    reported name, the table [2, n] (None for a band call) and the final list."""
    g = gpu
    d = Dev(g, setup=ms.tc_setup(g, "one_level" if s.get("one_level") else "default"))
    ctx = d.ctx
    assert d.pd.nlevels == (1 if s.get("one_level") else 2)
    if s.get("fast"):
        from kltamd.device import FAST
        d.td.reduction = FAST
    if "lazy" in s:
        d.ok(g.klt_hip_set_lazy_grad(ctx, s["lazy"]), "lazy_grad")
    x, y, v = start_list()
    n = len(x)
    dfr = d.up(np.stack(ms.scene(7)[:NF]))
    dx, dy, dv = d.up(x), d.up(y), d.up(v)
    tx, ty, tv = (d.up(np.zeros((NF - 1) * n, F32)) for _ in range(3))
    if s.get("planes") or s.get("planes_kept"):
        d.ok(g.klt_hip_set_path(ctx, 1), "path")
    d.ok(g.klt_hip_frames_begin(ctx, C.byref(d.pd), dfr, W), "begin")
    if s.get("planes_kept"):
        d.ok(g.klt_hip_set_path(ctx, 0), "path")
    if s.get("fb"):
        d.ok(g.klt_hip_set_fb(ctx, 1, FB_DIST), "fb")
    if s.get("pred"):
        d.ok(g.klt_hip_set_predict(ctx, 1, d.up(np.zeros(n, F32)), d.up(np.zeros(n, F32))), "predict")
    if s.get("mask"):
        d.ok(g.klt_hip_set_mask(ctx, d.up(np.full((H, W), 255, np.uint8)), W, MASK_TRACK), "mask")
    if s.get("times"):
        cap = 64
        buf = np.zeros(4 + 2 * cap, np.uint64)
        buf[2] = cap
        d.ok(g.klt_hip_set_wave_times(ctx, d.up(buf)), "wave_times")
    chunk = 4
    if s.get("exits"):  # two chunks, the second build released when no wave of the first tracker is left
        d.ok(g.klt_hip_set_frames_overlap(ctx, 3), "overlap")
        d.ok(g.klt_hip_set_frames_tail(ctx, 0), "tail")
        chunk = 1
    rest = dfr + W * H
    if s.get("band"):
        esc = d.up(np.zeros(1, np.int32))
        d.ok(g.klt_hip_track_frames_band(ctx, C.byref(d.pd), C.byref(d.td), rest, W, W * H, NF - 1, dx, dy, dv, n,
                                         -np.inf, np.inf, 0, H, esc, None, 0), "band")
        assert d.down(esc, 1, np.int32)[0] == 0
        table = None
    else:
        d.ok(g.klt_hip_track_frames(ctx, C.byref(d.pd), C.byref(d.td), rest, W, W * H, NF - 1, chunk, dx, dy, dv, n, tx,
                                    ty, tv, n), "frames")
        table = (d.down(tx, (NF - 1, n), F32), d.down(ty, (NF - 1, n), F32), d.down(tv, (NF - 1, n), np.int32))
    name = d.kernel().decode()
    final = (d.down(dx, n, F32), d.down(dy, n, F32), d.down(dv, n, np.int32))
    # nothing of this case stays with the context, which frees its buffers now
    d.ok(g.klt_hip_set_wave_times(ctx, None), "wave_times")
    d.ok(g.klt_hip_set_mask(ctx, None, 0, 0), "mask")
    d.ok(g.klt_hip_set_predict(ctx, 0, None, None), "predict")
    d.ok(g.klt_hip_set_fb(ctx, 0, 0.0), "fb")
    d.close()
    return name, table, final


def same_bits(got, want, what):
    for a, b, k in zip(got, want, "xyv"):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


@pytest.mark.parametrize("row", TRACK_ROWS, ids=case_id)
def test_tracker_row(gpu, oracle, row):
    want_name, s = row
    name, table, final = track(gpu, s)
    print(s, "->", name)
    assert name == want_name
    if s.get("fast"):
        return
    cfg = "one_level" if s.get("one_level") else "default"
    if s.get("fb"):
        x, y, v = start_list()
        exp = fb_want(oracle, ("instance names", cfg), ms.scene(7)[:NF], len(x), FB_DIST,
                      params=ms.oracle_params(oracle, cfg), start=(x, y, v))
        want = tuple(np.ascontiguousarray(exp[k][:, :NF - 1].T) for k in range(3))
    else:
        want = tuple(a[:NF - 1, PICK] for a in ms.oracle_placed(oracle, 7, cfg))
    assert (want[2][-1] == 0).sum() >= 10 and (want[2][-1] < 0).sum() >= 3  # tracked and lost features both
    rows = 1 if s.get("pred") else NF - 1
    if table is not None:
        same_bits([a[:rows] for a in table], [a[:rows] for a in want], "table")
    if rows == NF - 1:
        same_bits(final, [a[-1] for a in want], "final list")


def test_multi_rows(gpu, oracle):
    """k_track7_multi<2> and <0>: scenes 7 and 8 in one call, each against the oracle."""
    x, y, v = start_list()
    for cfg, name in (("default", K + "k_track7_multi<2>"), ("one_level", K + "k_track7_multi<0>")):
        d = Dev(gpu, setup=ms.tc_setup(gpu, cfg))
        got = d.multi([ms.scene(7), ms.scene(8)], [(x, y, v), (x, y, v)])
        assert d.kernel().decode() == name
        d.close()
        for g, seed in zip(got, ms.SCENES):
            same_bits(g[:3], [a[:, PICK] for a in ms.oracle_placed(oracle, seed, cfg)], (cfg, seed))


# ---------------------------------------------------------------------------
# the trackability map's seven names
# ---------------------------------------------------------------------------
E = "kltdev::(anonymous namespace)::"


def test_map_rows(gpu):
    from gpu_helpers import Dev as StageDev
    from kltamd.device import D2D, D2H, H2D, SelectDesc, check
    img = ms.scene(7)[0]
    border = 24
    for skip in (0, 1):
        def setup(t):
            t.borderx = t.bordery = border
            t.nSkippedPixels = skip
        d = StageDev(gpu, setup)
        lib, ctx = gpu, d.ctx
        d.build(img, slot=0)
        assert d.path(0) == 1  # fused: level 0 is records
        vals, nx, ny = d.eigen(0)
        assert lib.klt_hip_eigen_kernel(ctx).decode() == E + "k_min_eigen7<%d>" % (skip + 1)
        assert (vals > 0).sum() > nx * ny // 2  # a map with content
        sd = SelectDesc(7, 7, border, border, skip)
        dmap = lib.klt_hip_malloc(ctx, 4 * nx * ny)
        got = np.empty(nx * ny, np.int32)
        # from the image plane alone
        plane = np.empty((H, W), F32)
        check(lib, ctx, lib.klt_hip_download_level(ctx, 0, 0, 0, plane.ctypes.data), "level")
        dimg = lib.klt_hip_malloc(ctx, plane.nbytes)
        check(lib, ctx, lib.klt_hip_memcpy(ctx, dimg, plane.ctypes.data, plane.nbytes, H2D), "h2d")
        check(lib, ctx, lib.klt_hip_min_eigen_plane(ctx, dimg, W, H, C.byref(sd), dmap), "plane")
        assert lib.klt_hip_eigen_kernel(ctx).decode() == E + "k_min_eigen7_img<%d>" % (skip + 1)
        check(lib, ctx, lib.klt_hip_memcpy(ctx, got.ctypes.data, dmap, got.nbytes, D2H), "d2h")
        assert got.tobytes() == vals.tobytes()
        # from a frame of records
        fs = 3 * W * H
        drec = lib.klt_hip_malloc(ctx, 4 * fs)
        check(lib, ctx, lib.klt_hip_memcpy(ctx, drec, lib.klt_hip_level_ptr(ctx, 0, 0, 0), 4 * fs, D2D), "d2d")
        which = (C.c_int * 1)(0)
        got[:] = 0
        check(lib, ctx, lib.klt_hip_min_eigen_records(ctx, drec, fs, which, 1, W, H, C.byref(sd), dmap), "records")
        assert lib.klt_hip_eigen_kernel(ctx).decode() == E + "k_min_eigen7_multi<%d>" % (skip + 1)
        check(lib, ctx, lib.klt_hip_memcpy(ctx, got.ctypes.data, dmap, got.nbytes, D2H), "d2h")
        assert got.tobytes() == vals.tobytes()
        for p in (dmap, dimg, drec):
            lib.klt_hip_free(ctx, p)
        d.close()

    # the generic kernel: a step of 3, and a 9x9 window
    def step3(t):
        t.borderx = t.bordery = border
        t.nSkippedPixels = 2

    def win9(t):
        t.borderx = t.bordery = border
        t.window_width = t.window_height = 9

    for setup in (step3, win9):
        d = StageDev(gpu, setup)
        d.build(img, slot=0)
        vals, nx, ny = d.eigen(0)
        assert gpu.klt_hip_eigen_kernel(d.ctx).decode() == E + "k_min_eigen"
        assert (vals > 0).sum() > nx * ny // 2
        d.close()
