"""Lost features replaced inside the multi-sequence batched call
(klt_hip_track_frames_multi_replace, KLTTrackSequencesReplace) and the
trackability maps of several frames in one launch (k_min_eigen7_multi).

Sequences share nothing, so the batch is defined exactly: for every sequence,
what klt_hip_frames_begin + klt_hip_set_frames_replace + klt_hip_track_frames
give on a context of its own.  Every case compares x, y, val, the table rows,
the changed marks and the counters byte for byte with those separate calls of
the same session, and the table rows with the CPU oracle's loop

    track frame; if (count % every == 0) replace; store

Each case asserts its own condition (slots filled, a saturated frame, nothing
lost while others replace) from the oracle's run, so a case that stops being
real fails.

Common shape (tests/test_gpu_multi.py's): 160x120 frames, 13 tracked frames in
chunks of 4 -- four chunks, the last one ragged, every bank reused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import fl_affine, fl_to_arrays, u8ptr
from test_gpu_multi import Dev
from test_gpu_replace import frames_of, oracle_loop, same

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, T, CHUNK = 160, 120, 13, 4
MAP_KERNEL = b"kltdev::(anonymous namespace)::k_min_eigen7_multi<%d>"
TRACK_KERNEL = b"kltdev::k_track7_multi<2>"
# boundaries at features 60, 67, 67, 367, 407: all but the first inside 4-feature workgroups
MAIN = [(160120, 60), (72, 7), (73, 0), (160120, 300), (71, 40), (73, 1)]
PAIR = [(160120, 60), (71, 40)]

_singles = {}


def oracle_of(gpu, oracle, seed, n, every, frames=None, key=None):
    """oracle_loop, and what it would give for an empty list."""
    fr = frames if frames is not None else frames_of(gpu, seed)
    if n == 0:
        nt = len(fr) - 1
        none = (np.empty(0, F32), np.empty(0, F32), np.empty(0, np.int32))
        table = (np.empty((nt, 0), F32), np.empty((nt, 0), F32), np.empty((nt, 0), np.int32))
        return none, table, [(i, 0, 0) for i in range(every, nt + 1, every)]
    return oracle_loop(oracle, seed if key is None else key, fr, n, every)


def replace_desc(d, every, sel=None):
    """The description KLTTrackSequenceReplace passes; sel: another window, borders and step."""
    from kltamd.device import ReplaceDesc, SelectDesc
    rd = ReplaceDesc.from_tc(d.tc.contents, every)
    if sel:
        rd.sel = SelectDesc(*sel)
    return rd


def single(gpu, key, fr, start, every, fmt=0, sel=None):
    """One sequence on a context of its own with the setting on: table and list
    (as Dev.single), the counters (runs, filled) and the changed marks.
    Computed once per key."""
    if key not in _singles:
        n, nt = len(start[0]), len(fr) - 1
        d = Dev(gpu)
        ctx = d.ctx
        d.ok(gpu.klt_hip_set_frame_format(ctx, fmt), "format")
        rd = replace_desc(d, every, sel)
        d.ok(gpu.klt_hip_set_frames_replace(ctx, C.byref(rd)), "replace on")
        stack = np.stack(fr)
        pitch = stack.shape[2]
        fs = stack.shape[1] * pitch
        dfr = d.up(stack)
        dx, dy, dv = d.up(start[0]), d.up(start[1]), d.up(start[2])
        tx, ty, tv = (d.up(np.zeros(nt * max(n, 1), F32)) for _ in range(3))
        d.ok(gpu.klt_hip_frames_begin(ctx, C.byref(d.pd), dfr, pitch), "begin")
        d.ok(gpu.klt_hip_track_frames(ctx, C.byref(d.pd), C.byref(d.td), dfr + fs, pitch, fs, nt, CHUNK, dx, dy, dv, n,
                                      tx, ty, tv, n), "frames")
        out = (d.down(tx, (nt, n), F32), d.down(ty, (nt, n), F32), d.down(tv, (nt, n), np.int32),
               d.down(dx, n, F32), d.down(dy, n, F32), d.down(dv, n, np.int32))
        cnt, runs, filled = C.c_long(), C.c_long(), C.c_long()
        d.ok(gpu.klt_hip_get_frames_replace(ctx, None, C.byref(cnt), C.byref(runs), C.byref(filled)), "get")
        assert cnt.value == nt
        changed = np.zeros(n, np.uint8)
        d.ok(gpu.klt_hip_frames_replace_changed(ctx, changed.ctypes.data, n), "changed")
        d.close()
        _singles[key] = (out, (runs.value, filled.value), changed)
    return _singles[key]


class Batch:
    """The device arrays of one batch and klt_hip_track_frames_multi_replace
    calls on them.  one_block: x | y | val in one allocation (a replacement
    moves them in one transfer), else three."""

    def __init__(self, d, seqs, starts, frame_major=False, one_block=True):
        self.d, self.gpu, self.starts = d, d.gpu, starts
        self.S = S = len(seqs)
        x, y, v = self.first = tuple(np.concatenate([s[k] for s in starts]) for k in range(3))
        self.n = n = len(x)
        stack = np.stack([np.stack(f) for f in seqs])  # [S, nt + 1, H, pitch]
        self.nt = nt = stack.shape[1] - 1
        self.pitch = stack.shape[3]
        fs = stack.shape[2] * self.pitch
        if frame_major:
            stack = np.ascontiguousarray(stack.transpose(1, 0, 2, 3))
            self.stride, self.seq_stride = S * fs, fs
        else:
            self.stride, self.seq_stride = fs, (nt + 1) * fs
        self.dfr = d.up(stack)
        if one_block:
            self.dx = d.up(np.concatenate([x.view(np.int32), y.view(np.int32), v]))
            self.dy, self.dv = self.dx + 4 * n, self.dx + 8 * n
        else:
            self.dx, self.dy, self.dv = d.up(x), d.up(y), d.up(v)
        self.tab = [d.up(np.zeros(nt * max(n, 1), F32)) for _ in range(3)]
        self.changed = np.zeros(max(n, 1), np.uint8)
        self.runs, self.filled = (C.c_long * S)(), (C.c_long * S)()
        self.counts = (C.c_int * S)(*[len(s[0]) for s in starts])

    def call(self, rd, count0=0, j=0, nf=None, chunk=CHUNK, td=None):
        d, n = self.d, self.n
        off = 4 * j * n
        return self.gpu.klt_hip_track_frames_multi_replace(
            d.ctx, C.byref(d.pd), C.byref(td if td is not None else d.td), C.byref(rd) if rd is not None else None,
            count0, self.dfr + j * self.stride, self.pitch, self.stride, self.seq_stride, self.S,
            self.nt if nf is None else nf, chunk, self.counts, self.dx, self.dy, self.dv, self.tab[0] + off,
            self.tab[1] + off, self.tab[2] + off, n, self.changed.ctypes.data, self.runs, self.filled)

    def lists(self):
        d, n = self.d, self.n
        return d.down(self.dx, n, F32), d.down(self.dy, n, F32), d.down(self.dv, n, np.int32)

    def results(self):
        """Per sequence what single() returns."""
        d, n, nt = self.d, self.n, self.nt
        X, Y, V = (d.down(t, (nt, n), dt) for t, dt in zip(self.tab, (F32, F32, np.int32)))
        x, y, v = self.lists()
        out, a = [], 0
        for s, st in enumerate(self.starts):
            b = a + len(st[0])
            arrays = tuple(np.ascontiguousarray(q[..., a:b]) for q in (X, Y, V, x, y, v))
            out.append((arrays, (self.runs[s], self.filled[s]), self.changed[a:b].copy()))
            a = b
        return out


def run_batch(gpu, seqs, starts, every, chunk=CHUNK, calls=None, budget=None, fmt=0, sel=None, **layout):
    """The whole batch in one call (or in `calls` pieces, the count running on);
    the per-sequence results, the kernels and the chunk used."""
    d = Dev(gpu, budget=budget)
    d.ok(gpu.klt_hip_set_frame_format(d.ctx, fmt), "format")
    b = Batch(d, seqs, starts, **layout)
    rd = replace_desc(d, every, sel)
    j = 0
    for nf in calls or [b.nt]:
        d.ok(b.call(rd, count0=j, j=j, nf=nf, chunk=chunk), "multi_replace")
        j += nf
    assert j == b.nt
    out = b.results()
    info = (gpu.klt_hip_eigen_kernel(d.ctx), d.kernel(), gpu.klt_hip_frames_chunk(d.ctx))
    d.close()
    return out, info


def the_same(got, want):
    (g, gc, gm), (w, wc, wm) = got, want
    same(g, w)
    assert tuple(gc) == tuple(wc)  # runs, filled
    assert gm.tobytes() == wm.tobytes()  # changed


def case_of(gpu, oracle, pairs, every):
    """Frames, the oracle's starts, tables and points, and the separate calls."""
    seqs = [frames_of(gpu, s) for s, _ in pairs]
    orc = [oracle_of(gpu, oracle, s, n, every) for s, n in pairs]
    starts = [o[0] for o in orc]
    refs = [single(gpu, (s, n, every), fr, st, every) for (s, n), fr, st in zip(pairs, seqs, starts)]
    for (out, (runs, filled), changed), (_, table, points) in zip(refs, orc):
        same(out[:3], table)  # the separate call is the oracle's loop
        assert runs == sum(1 for _, lost, _ in points if lost) and filled == sum(p[2] for p in points)
    return seqs, starts, orc, refs


def check_main(orc):
    """What makes the main batch what it is, from the oracle's runs (every = 3)."""
    points = {pair: o[2] for pair, o in zip(MAIN, orc)}
    assert all([p[0] for p in pts] == [3, 6, 9, 12] for pts in points.values())
    assert [p[2] for p in points[160120, 60]] == [7, 5, 5, 3]
    assert all(241 <= lost <= 246 and 5 <= filled <= 8 for _, lost, filled in points[160120, 300])  # saturated
    assert [p[2] for p in points[71, 40]] == [4, 5, 1, 1]
    # the per-sequence early-out while others replace
    assert [p[1] > 0 for p in points[72, 7]] == [False, True, False, False]
    assert [p[2] for p in points[72, 7]] == [0, 1, 0, 0]
    assert all(lost == 0 for _, lost, _ in points[73, 1])


# ---------------------------------------------------------------------------
# 1. the batch against the separate calls and the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frame_major", [False, True])
def test_main_batch(gpu, oracle, frame_major):
    seqs, starts, orc, refs = case_of(gpu, oracle, MAIN, 3)
    check_main(orc)
    got, (eig, kernel, chunk) = run_batch(gpu, seqs, starts, 3, frame_major=frame_major)
    assert eig == MAP_KERNEL % 1 and kernel == TRACK_KERNEL and chunk == CHUNK
    for g, r, o in zip(got, refs, orc):
        the_same(g, r)
        same(g[0][:3], o[1])
    assert [g[1] for g in got] == [(4, 20), (1, 1), (0, 0), (4, sum(p[2] for p in orc[3][2])), (4, 11), (0, 0)]
    assert not got[5][2].any() and got[0][2].sum() >= 7  # the marks: none for (73, 1), the filled slots for (160120, 60)


@pytest.mark.parametrize("every", [1, 4, 64])
def test_every(gpu, oracle, every):
    seqs, starts, orc, refs = case_of(gpu, oracle, PAIR, every)
    a, b = orc[0][2], orc[1][2]
    if every == 1:
        assert [i for i, lost, _ in b if lost == 0] == [7, 8, 9, 10, 12, 13]  # nothing lost there ...
        assert len(a) == T and all(filled > 0 for _, _, filled in a)       # ... while the other fills at every frame
    elif every == 4:
        assert [p[0] for p in a] == [4, 8, 12] and all(p[2] > 0 for p in a)
    else:
        assert not a and not b
    # three list arrays at every = 4, one block otherwise: both ways of moving the lists
    got, (eig, kernel, _) = run_batch(gpu, seqs, starts, every, one_block=every != 4)
    for g, r, o in zip(got, refs, orc):
        the_same(g, r)
        same(g[0][:3], o[1])
    if every == 64:  # no replacement inside the sequence: the plain multi call
        assert eig == b"" and all(g[1] == (0, 0) and not g[2].any() for g in got)
        d = Dev(gpu)
        plain = d.multi(seqs, starts)
        d.close()
        for g, p in zip(got, plain):
            same(g[0], p)
    else:
        assert eig == MAP_KERNEL % 1 and kernel == TRACK_KERNEL


@pytest.mark.parametrize("chunk,budget", [(1, None), (4, None), (64, None), (4, 8_000_000)])
def test_chunk_independence(gpu, oracle, chunk, budget):
    seqs, starts, _, refs = case_of(gpu, oracle, MAIN, 3)
    got, (_, _, used) = run_batch(gpu, seqs, starts, 3, chunk=chunk, budget=budget, frame_major=chunk == 1)
    if budget:  # 8 MB hold at most nine 160x120 pyramids per bank: less than two groups of six
        assert used == 1
    else:
        assert used == chunk
    for g, r in zip(got, refs):
        the_same(g, r)


def test_split_calls_equal_one_call(gpu, oracle):
    seqs, starts, _, refs = case_of(gpu, oracle, MAIN, 3)
    got, _ = run_batch(gpu, seqs, starts, 3, calls=[3, 4, 6])  # count0 = 0, 3, 7
    for g, r in zip(got, refs):
        the_same(g, r)


def test_colour_frames(gpu, oracle):
    from kltamd.device import FRAME_BGR8
    from test_gpu_frame_format import colour, expected_gray
    every, seqs, starts, refs, orc = 3, [], [], [], []
    for seed, n in PAIR:
        gray = [np.ascontiguousarray(expected_gray(f)) for f in frames_of(gpu, seed)]
        bgr = [colour(f, FRAME_BGR8) for f in frames_of(gpu, seed)]
        o = oracle_loop(oracle, ("bgr", seed), gray, n, every)
        assert len(o[2]) == 4 and sum(filled > 0 for _, _, filled in o[2]) >= 3
        seqs.append(bgr)
        starts.append(o[0])
        orc.append(o)
        refs.append(single(gpu, ("bgr", seed, n, every), bgr, o[0], every, fmt=FRAME_BGR8))
    got, (eig, kernel, _) = run_batch(gpu, seqs, starts, every, fmt=FRAME_BGR8, frame_major=True)
    assert eig == MAP_KERNEL % 1 and kernel == TRACK_KERNEL
    for g, r, o in zip(got, refs, orc):
        the_same(g, r)
        same(g[0][:3], o[1])


def test_more_sequences_than_xcds(gpu, oracle):
    pairs = [(s, 40) for s in (160120, 71, 72, 73, 74, 75, 76, 77, 78)]
    seqs, starts, orc, refs = case_of(gpu, oracle, pairs, 3)
    for (seed, _), o in zip(pairs, orc):
        if seed >= 75:
            assert len(o[2]) == 4 and all(filled > 0 for _, _, filled in o[2]), seed
    got, _ = run_batch(gpu, seqs, starts, 3)
    for g, r, o in zip(got, refs, orc):
        the_same(g, r)
        same(g[0][:3], o[1])


@pytest.mark.parametrize("sel", [(9, 9, 24, 24, 0), (7, 7, 24, 24, 2)])
def test_a_description_the_map_kernel_does_not_cover(gpu, oracle, sel):
    """A selection window other than 7x7 or a step above 2 cannot come from the
    tracking context the call covers, but the description is an argument of its
    own: the maps then come from one k_min_eigen launch per sequence."""
    seqs, starts, _, _ = case_of(gpu, oracle, PAIR, 3)
    refs = [single(gpu, (s, n, 3, sel), fr, st, 3, sel=sel) for (s, n), fr, st in zip(PAIR, seqs, starts)]
    assert all(runs >= 1 and filled >= 1 for _, (runs, filled), _ in refs)  # every sequence has lost a slot by frame 3
    got, (eig, kernel, _) = run_batch(gpu, seqs, starts, 3, sel=sel)
    assert eig == b"kltdev::(anonymous namespace)::k_min_eigen" and kernel == TRACK_KERNEL
    for g, r in zip(got, refs):
        the_same(g, r)


# ---------------------------------------------------------------------------
# 2. the kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,border,skip", [(70, 40, 3, 0), (160, 120, 24, 0), (160, 120, 24, 1), (333, 251, 24, 0)])
def test_maps_of_record_frames_equal_the_single_maps(gpu, w, h, border, skip):
    from gpu_helpers import Dev as StageDev
    from kltamd.device import D2D, D2H, SelectDesc, check

    def setup(t):
        t.borderx = t.bordery = border
        t.nSkippedPixels = skip

    d = StageDev(gpu, setup)
    lib, ctx = gpu, d.ctx
    want = []
    for slot, img in enumerate(synth(gpu, 7100 + w, w, h, 3)):  # three different images
        d.build(img, slot=slot)
        assert d.path(slot) == 1 and lib.klt_hip_level_interleaved(ctx, slot, 0) == 1  # a fused slot: records
        vals, nx, ny = d.eigen(slot)
        assert b"k_min_eigen7<" in lib.klt_hip_eigen_kernel(ctx)
        assert (vals > 0).sum() > nx * ny // 2  # a map with content
        want.append(vals)
    assert want[0].tobytes() != want[2].tobytes()
    fs = 3 * w * h  # floats per frame of records
    drec = lib.klt_hip_malloc(ctx, 3 * 4 * fs)
    dmaps = lib.klt_hip_malloc(ctx, 2 * 4 * nx * ny)
    for slot in range(3):
        check(lib, ctx, lib.klt_hip_memcpy(ctx, drec + slot * 4 * fs, lib.klt_hip_level_ptr(ctx, slot, 0, 0), 4 * fs,
                                           D2D), "d2d")
    sd = SelectDesc(7, 7, border, border, skip)
    which = (C.c_int * 2)(2, 0)  # a subset, out of order
    check(lib, ctx, lib.klt_hip_min_eigen_records(ctx, drec, fs, which, 2, w, h, C.byref(sd), dmaps), "records")
    assert lib.klt_hip_eigen_kernel(ctx) == MAP_KERNEL % (skip + 1)
    got = np.empty((2, nx * ny), np.int32)
    check(lib, ctx, lib.klt_hip_memcpy(ctx, got.ctypes.data, dmaps, got.nbytes, D2H), "d2h")
    assert got[0].tobytes() == want[2].tobytes()
    assert got[1].tobytes() == want[0].tobytes()
    for bad, nsel in ((SelectDesc(9, 9, border + 1, border + 1, 0), 2), (SelectDesc(7, 7, border, border, 2), 2),
                      (SelectDesc(7, 7, 2, border, 0), 2), (sd, 0), (sd, 65)):
        assert lib.klt_hip_min_eigen_records(ctx, drec, fs, which, nsel, w, h, C.byref(bad), dmaps) == -1
        assert lib.klt_hip_last_error(ctx)
    lib.klt_hip_free(ctx, drec)
    lib.klt_hip_free(ctx, dmaps)
    d.close()


# ---------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu, oracle):
    from kltamd.device import ReplaceDesc, SelectDesc
    seqs, starts, _, _ = case_of(gpu, oracle, PAIR, 3)
    d = Dev(gpu)
    ctx = d.ctx
    b = Batch(d, seqs, starts)
    good = replace_desc(d, 3)

    def refused(what, rd=good, word=b"track_frames_multi_replace", **kw):
        assert b.call(rd, **kw) == -1, what
        assert word in d.error(), (what, d.error())
        assert d.kernel() == b"" and gpu.klt_hip_eigen_kernel(ctx) == b"", what  # no launch so far
        same(b.lists(), b.first)
        assert not b.changed.any() and not any(b.runs) and not any(b.filled), what

    refused("no description", rd=None)
    refused("every 0", rd=ReplaceDesc(good.sel, 10, 1, 0), word=b"every")
    refused("border below the window's half size", rd=ReplaceDesc(SelectDesc(7, 7, 2, 24, 0), 10, 1, 3), word=b"border")
    refused("window 0", rd=ReplaceDesc(SelectDesc(0, 7, 24, 24, 0), 10, 1, 3), word=b"window")
    refused("negative nSkippedPixels", rd=ReplaceDesc(SelectDesc(7, 7, 24, 24, -1), 10, 1, 3), word=b"nSkippedPixels")
    refused("negative count0", count0=-1, word=b"count0")
    d.ok(gpu.klt_hip_set_frames_replace(ctx, C.byref(good)), "setting on")
    refused("the context's setting", word=b"klt_hip_set_frames_replace")
    d.ok(gpu.klt_hip_set_frames_replace(ctx, None), "setting off")
    d.ok(gpu.klt_hip_set_fb(ctx, 1, 0.5), "fb on")
    refused("forward-backward check", word=b"forward-backward")
    d.ok(gpu.klt_hip_set_fb(ctx, 0, 0.0), "fb off")
    refused("chunk 0", chunk=0)
    # and with everything off again the same call tracks and replaces
    d.ok(b.call(good), "multi_replace")
    assert d.kernel() == TRACK_KERNEL and gpu.klt_hip_eigen_kernel(ctx) == MAP_KERNEL % 1
    assert b.changed.any() and all(b.runs) and all(b.filled)
    # the plain multi call still refuses the context's setting
    d.ok(gpu.klt_hip_set_frames_replace(ctx, C.byref(good)), "setting on")
    rc, _, _ = d.multi_call(seqs, starts)
    assert rc == -1 and b"klt_hip_set_frames_replace" in d.error()
    d.close()


# ---------------------------------------------------------------------------
# 4. KLTTrackSequencesReplace
# ---------------------------------------------------------------------------
def ft_arrays(ft, nfeat, col0, ncol):
    cell = lambda j, i: ft.contents.feature[j][i].contents  # noqa: E731
    return tuple(np.array([[getattr(cell(j, col0 + i), f) for i in range(ncol)] for j in range(nfeat)], dt)
                 for f, dt in (("x", F32), ("y", F32), ("val", np.int32)))


def klt_sequences(gpu, pairs, every, together, tables, ft_col, nframes=T + 1, sequential=True):
    """Select on each sequence's frame 0, then KLTTrackSequencesReplace
    (together; every None: KLTTrackSequences) or the loop of
    KLTTrackSequenceReplace on a fresh context per sequence: per sequence the
    final list, its affine state and the table; the kernels of tc's device."""
    from kltamd.abi import FL, FT
    nt = nframes - 1
    U8P = C.POINTER(C.c_ubyte)
    keep = [frames_of(gpu, s, n=nframes) for s, _ in pairs]
    arrs = [(U8P * nframes)(*[u8ptr(f) for f in fr]) for fr in keep]
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1 if sequential else 0
    fls, fts = [], []
    for fr, (_, n) in zip(keep, pairs):
        sel = gpu.KLTCreateTrackingContext()
        fl = gpu.KLTCreateFeatureList(n)
        gpu.KLTSelectGoodFeatures(sel, u8ptr(fr[0]), W, H, fl)
        gpu.KLTFreeTrackingContext(sel)
        fls.append(fl)
        fts.append(gpu.KLTCreateFeatureTable(nt + ft_col, n) if tables else None)
    if together:
        S = len(pairs)
        frames = (C.POINTER(U8P) * S)(*[C.cast(a, C.POINTER(U8P)) for a in arrs])
        fl_arr = (FL * S)(*fls)
        ft_arr = (FT * S)(*fts) if tables else None
        if every is None:
            gpu.KLTTrackSequences(tc, frames, S, nframes, W, H, fl_arr, ft_arr, ft_col)
        else:
            gpu.KLTTrackSequencesReplace(tc, frames, S, nframes, W, H, fl_arr, ft_arr, ft_col, every)
    else:
        for arr, fl, ft in zip(arrs, fls, fts):
            t = gpu.KLTCreateTrackingContext()
            t.contents.sequentialMode = 1 if sequential else 0
            gpu.KLTTrackSequenceReplace(t, arr, nframes, W, H, fl, ft, ft_col, every)
            gpu.KLTFreeTrackingContext(t)
    ctx = gpu.klt_amd_device_context(tc)
    kernels = (gpu.klt_hip_track_kernel(ctx), gpu.klt_hip_eigen_kernel(ctx))
    out = []
    for fl, ft, (_, n) in zip(fls, fts, pairs):
        out.append(fl_to_arrays(fl) + fl_affine(fl) + (ft_arrays(ft, n, ft_col, nt) if ft else ()))
        gpu.KLTFreeFeatureList(fl)
        if ft:
            gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeTrackingContext(tc)
    return out, kernels


KLT_PAIRS = [(160120, 60), (72, 7), (71, 40)]


@pytest.mark.parametrize("tables,ft_col", [(False, 0), (True, 0), (True, 2)])
def test_klt_sequences_replace_equals_the_loop(gpu, tables, ft_col):
    want, _ = klt_sequences(gpu, KLT_PAIRS, 3, False, tables, ft_col)
    got, kernels = klt_sequences(gpu, KLT_PAIRS, 3, True, tables, ft_col)
    assert kernels == (TRACK_KERNEL, MAP_KERNEL % 1)  # tracked and replaced together, not by the fallback loop
    for g, w in zip(got, want):
        same(g, w)
    assert sum((w[2] >= 0).sum() for w in want) > 60
    if not tables:  # the case is real: without the replacements the lists end differently
        plain, _ = klt_sequences(gpu, KLT_PAIRS, None, True, False, 0)
        assert plain[0][2].tobytes() != got[0][2].tobytes() and (plain[0][2] >= 0).sum() < (got[0][2] >= 0).sum()


def test_klt_sequences_replace_longer_than_a_group(gpu):
    """21 frames: two groups of tracked frames (16 + 4), replacements at 5, 10,
    15 and 20 -- the count runs on through the groups."""
    pairs = [(160120, 60), (71, 40)]
    want, _ = klt_sequences(gpu, pairs, 5, False, True, 0, nframes=21)
    got, kernels = klt_sequences(gpu, pairs, 5, True, True, 0, nframes=21)
    assert kernels == (TRACK_KERNEL, MAP_KERNEL % 1)
    for g, w in zip(got, want):
        same(g, w)
    V = want[0][8]  # [n, frames]: a slot lost at frame 19 that the replacement at frame 20, in the second group, filled
    assert ((V[:, 18] < 0) & (V[:, 19] >= 0)).any()


def test_klt_sequences_replace_falls_back_without_sequential_mode(gpu):
    want, _ = klt_sequences(gpu, KLT_PAIRS, 3, False, True, 1, sequential=False)
    got, kernels = klt_sequences(gpu, KLT_PAIRS, 3, True, True, 1, sequential=False)
    assert kernels[0] != TRACK_KERNEL
    for g, w in zip(got, want):
        same(g, w)
    assert sum((w[2] >= 0).sum() for w in want) > 60
