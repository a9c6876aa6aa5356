"""Several independent sequences in one batched call
(klt_hip_track_frames_multi, KLTTrackSequences).

Sequences share nothing, so a batch is defined exactly: what the separate
single-sequence calls give.  Every case compares x, y, val and the table rows
byte for byte with klt_hip_frames_begin + klt_hip_track_frames runs of the same
session; one sequence is held to the oracle as well.

Common shape (tests/test_gpu_schedule.py's): 160x120 frames, 13 tracked frames
in chunks of 4 -- four chunks, the last one ragged, every bank reused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import OracleTracker, fl_to_arrays, u8ptr

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, T, CHUNK = 160, 120, 13, 4
OOB = -4
MULTI_KERNEL = b"kltdev::k_track7_multi<2>"
SEEDS = [160120, 71, 72, 73, 74, 75, 76, 77, 78]

_frames, _starts, _singles = {}, {}, {}


def frames_of(gpu, seed):
    if seed not in _frames:
        _frames[seed] = synth(gpu, seed, W, H, T + 1)
    return _frames[seed]


def empty():
    return np.empty(0, F32), np.empty(0, F32), np.empty(0, np.int32)


def start_of(gpu, seed, n):
    """KLTSelectGoodFeatures on the sequence's frame 0."""
    if (seed, n) not in _starts:
        if n == 0:
            _starts[seed, n] = empty()
        else:
            tc = gpu.KLTCreateTrackingContext()
            fl = gpu.KLTCreateFeatureList(n)
            gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(frames_of(gpu, seed)[0])), W, H, fl)
            _starts[seed, n] = fl_to_arrays(fl)
            gpu.KLTFreeFeatureList(fl)
            gpu.KLTFreeTrackingContext(tc)
    return _starts[seed, n]


class Dev:
    """A tracking context's device context with the default descriptors."""

    def __init__(self, gpu, budget=None, search_range=None, setup=None):
        from kltamd.device import PyrDesc, TrackDesc
        self.gpu = gpu
        self.tc = gpu.KLTCreateTrackingContext()
        self.tc.contents.sequentialMode = 1
        if setup:  # other fields of the tracking context record, before the descriptors are taken from it
            setup(self.tc.contents)
        if search_range is not None:
            gpu.KLTChangeTCPyramid(self.tc, search_range)
            gpu.KLTUpdateTCBorder(self.tc)
        self.ctx = gpu.klt_amd_device_context(self.tc)
        if budget is not None:
            assert gpu.klt_hip_set_bank_budget(self.ctx, budget) == 0
        self.pd, self.td = PyrDesc(), TrackDesc()
        gpu.klt_amd_pyr_desc(self.tc, W, H, self.tc.contents.nPyramidLevels, 1, C.byref(self.pd))
        gpu.klt_amd_track_desc(self.tc, C.byref(self.td))
        self.held = []

    def ok(self, rc, what):
        from kltamd.device import check
        check(self.gpu, self.ctx, rc, what)

    def up(self, a):
        from kltamd.device import H2D
        a = np.ascontiguousarray(a)
        d = self.gpu.klt_hip_malloc(self.ctx, max(a.nbytes, 4))
        assert d
        self.held.append(d)
        if a.nbytes:
            self.ok(self.gpu.klt_hip_memcpy(self.ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        return d

    def down(self, d, shape, dtype):
        from kltamd.device import D2H
        a = np.empty(shape, dtype)
        self.ok(self.gpu.klt_hip_sync(self.ctx), "sync")
        if a.nbytes:
            self.ok(self.gpu.klt_hip_memcpy(self.ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return a

    def kernel(self):
        return self.gpu.klt_hip_track_kernel(self.ctx)

    def error(self):
        return self.gpu.klt_hip_last_error(self.ctx)

    def close(self):
        for d in self.held:
            self.gpu.klt_hip_free(self.ctx, d)
        self.gpu.KLTFreeTrackingContext(self.tc)

    def single(self, frames, start, chunk=CHUNK, calls=None):
        """klt_hip_frames_begin on frames[0], one klt_hip_track_frames call over
        the rest (or one per entry of `calls`, that many frames each): the table
        [T, n] and the final list."""
        x, y, v = start
        n = len(x)
        dfr = self.up(np.stack(frames))
        dx, dy, dv = self.up(x), self.up(y), self.up(v)
        tx, ty, tv = (self.up(np.zeros(T * max(n, 1), F32)) for _ in range(3))
        self.ok(self.gpu.klt_hip_frames_begin(self.ctx, C.byref(self.pd), dfr, W), "begin")
        j = 0
        for nf in calls or [T]:
            off = 4 * j * n
            self.ok(self.gpu.klt_hip_track_frames(self.ctx, C.byref(self.pd), C.byref(self.td), dfr + (j + 1) * W * H,
                                                  W, W * H, nf, chunk, dx, dy, dv, n, tx + off, ty + off, tv + off,
                                                  n), "frames")
            j += nf
        assert j == T
        return (self.down(tx, (T, n), F32), self.down(ty, (T, n), F32), self.down(tv, (T, n), np.int32),
                self.down(dx, n, F32), self.down(dy, n, F32), self.down(dv, n, np.int32))

    def multi_call(self, seqs, starts, chunk=CHUNK, frame_major=False, td=None, nseq=None, counts=None,
                   tab_stride=None):
        """One klt_hip_track_frames_multi call; returns rc and the device
        arrays.  Frames sequence-major (one pair of pyramid launches per
        sequence) or frame-major (one pair per chunk)."""
        S = len(seqs)
        x, y, v = (np.concatenate([s[k] for s in starts]) for k in range(3))
        n = len(x)
        stack = np.stack([np.stack(f) for f in seqs])  # [S, T+1, H, W]
        if frame_major:
            stack = np.ascontiguousarray(stack.transpose(1, 0, 2, 3))
            stride, seq_stride = S * W * H, W * H
        else:
            stride, seq_stride = W * H, (T + 1) * W * H
        dfr = self.up(stack)
        dx, dy, dv = self.up(x), self.up(y), self.up(v)
        tx, ty, tv = (self.up(np.zeros(T * max(n, 1), F32)) for _ in range(3))
        n_seq = (C.c_int * max(S, 1))(*(counts if counts is not None else [len(s[0]) for s in starts]))
        rc = self.gpu.klt_hip_track_frames_multi(self.ctx, C.byref(self.pd), C.byref(td or self.td), dfr, W, stride,
                                                 seq_stride, S if nseq is None else nseq, T, chunk, n_seq, dx, dy, dv,
                                                 tx, ty, tv, n if tab_stride is None else tab_stride)
        return rc, n, (dx, dy, dv, tx, ty, tv)

    def multi(self, seqs, starts, **kw):
        """The call's results split per sequence, each like single()'s."""
        rc, n, (dx, dy, dv, tx, ty, tv) = self.multi_call(seqs, starts, **kw)
        self.ok(rc, "multi")
        X, Y, V = self.down(tx, (T, n), F32), self.down(ty, (T, n), F32), self.down(tv, (T, n), np.int32)
        x, y, v = self.down(dx, n, F32), self.down(dy, n, F32), self.down(dv, n, np.int32)
        out, a = [], 0
        for s in starts:
            b = a + len(s[0])
            out.append(tuple(np.ascontiguousarray(q[..., a:b]) for q in (X, Y, V, x, y, v)))
            a = b
        return out


def same(a, b):
    for p, q in zip(a, b):
        assert p.shape == q.shape
        assert p.tobytes() == q.tobytes()


def single_ref(gpu, seed, start_key, start):
    """One sequence on its own, on a context of its own, computed once."""
    if (seed, start_key) not in _singles:
        d = Dev(gpu)
        _singles[seed, start_key] = d.single(frames_of(gpu, seed), start)
        d.close()
    return _singles[seed, start_key]


def selected_case(gpu, counts):
    seeds = SEEDS[:len(counts)]
    seqs = [frames_of(gpu, s) for s in seeds]
    starts = [start_of(gpu, s, n) for s, n in zip(seeds, counts)]
    refs = [single_ref(gpu, s, n, st) for s, n, st in zip(seeds, counts, starts)]
    return seqs, starts, refs


COUNTS = [300, 0, 7, 1]  # an empty sequence; boundaries at features 300 and 307: inside 4-feature workgroups


@pytest.mark.parametrize("frame_major", [False, True])
def test_equals_the_separate_calls(gpu, oracle, frame_major):
    seqs, starts, refs = selected_case(gpu, COUNTS)
    d = Dev(gpu)
    got = d.multi(seqs, starts, frame_major=frame_major)
    assert d.kernel() == MULTI_KERNEL
    d.close()
    for g, r in zip(got, refs):
        same(g, r)
    assert (refs[0][2][-1] == 0).sum() > 10  # the case is real: features survive the sequence
    X, Y, V = got[0][:3]
    OX, OY, OV = OracleTracker(oracle).harness(seqs[0], 300, T + 1, first=seqs[0][0])
    for j in range(T):
        assert np.array_equal(V[j], OV[:, j])
        assert np.array_equal(X[j].view(np.int32), OX[:, j].view(np.int32))
        assert np.array_equal(Y[j].view(np.int32), OY[:, j].view(np.int32))


def test_chunk_independence(gpu):
    seqs, starts, refs = selected_case(gpu, COUNTS)
    for chunk in (1, 4, 64):
        d = Dev(gpu)
        got = d.multi(seqs, starts, chunk=chunk)
        assert gpu.klt_hip_frames_chunk(d.ctx) == chunk
        d.close()
        for g, r in zip(got, refs):
            same(g, r)
    # 8 MB hold at most nine 160x120 pyramids in each of the three banks: two groups of four
    d = Dev(gpu, budget=8_000_000)
    got = d.multi(seqs, starts, chunk=CHUNK)
    assert gpu.klt_hip_frames_chunk(d.ctx) == 2
    d.close()
    for g, r in zip(got, refs):
        same(g, r)


def test_tuning_hooks_do_not_change_the_bytes(gpu):
    seqs, starts, refs = selected_case(gpu, COUNTS)
    for hook, value in (("klt_hip_set_track_merge", 0), ("klt_hip_set_track_prio", 0), ("klt_hip_set_track_order", 1),
                        ("klt_hip_set_lazy_grad", 0), ("klt_hip_set_frames_overlap", 2)):
        d = Dev(gpu)
        d.ok(getattr(gpu, hook)(d.ctx, value), hook)
        got = d.multi(seqs, starts)
        d.close()
        for g, r in zip(got, refs):
            same(g, r)


def test_one_level_pyramid(gpu):
    """A search range of 2 gives a one-level pyramid (still the fused path):
    the runtime-depth instance."""
    seeds, counts = SEEDS[:3], [60, 7, 33]
    seqs = [frames_of(gpu, s) for s in seeds]
    starts = [start_of(gpu, s, n) for s, n in zip(seeds, counts)]
    refs = []
    for fr, st in zip(seqs, starts):
        d = Dev(gpu, search_range=2)
        assert d.pd.nlevels == 1
        refs.append(d.single(fr, st))
        d.close()
    assert sum((r[2][-1] == 0).sum() for r in refs) > 10
    d = Dev(gpu, search_range=2)
    got = d.multi(seqs, starts)
    assert d.kernel() == b"kltdev::k_track7_multi<0>"
    d.close()
    for g, r in zip(got, refs):
        same(g, r)


def test_no_cross_talk(gpu):
    a, b = SEEDS[0], SEEDS[1]
    start = start_of(gpu, a, 300)
    ra, rb = single_ref(gpu, a, 300, start), single_ref(gpu, b, "start of %d" % a, start)
    d = Dev(gpu)
    ga, gb = d.multi([frames_of(gpu, a), frames_of(gpu, b)], [start, start])
    same(ga, ra)
    same(gb, rb)
    assert ga[0].tobytes() != gb[0].tobytes()
    g1, g2 = d.multi([frames_of(gpu, a), frames_of(gpu, a)], [start, start])
    d.close()
    same(g1, ra)
    same(g2, ra)


def test_one_sequence(gpu):
    seqs, starts, refs = selected_case(gpu, [300])
    d = Dev(gpu)
    got = d.multi(seqs, starts)
    d.close()
    same(got[0], refs[0])


def test_more_sequences_than_xcds(gpu):
    seqs, starts, refs = selected_case(gpu, [5] * 9)
    assert sum((r[2][-1] == 0).sum() for r in refs) > 9
    for fm in (False, True):
        d = Dev(gpu)
        got = d.multi(seqs, starts, frame_major=fm)
        d.close()
        for g, r in zip(got, refs):
            same(g, r)


def test_losses_at_the_border(gpu):
    """Sequence 1 carries hand-placed features next to the tracking border
    (24 px) that the synthetic motion takes out of bounds within the 13 frames.
    Frame t samples the field at (x + 0.7 t, y + 0.3 t) (include/klt_synth.h),
    so the image content moves by (-0.7, -0.3) px per frame: the features
    placed at the left and top border leave, one after the other; the ones
    placed at the right and bottom border ride along and move inwards."""
    xs = np.concatenate([np.arange(24.5, 31.5, 0.5), np.full(10, 80.0),
                         np.arange(128.0, 135.0, 0.5), np.full(10, 80.0)]).astype(F32)
    ys = np.concatenate([np.full(14, 60.0), np.arange(24.25, 26.75, 0.25),
                         np.full(14, 60.0), np.arange(90.0, 95.0, 0.5)]).astype(F32)
    placed = (xs, ys, np.zeros(len(xs), np.int32))
    seeds = SEEDS[:3]
    starts = [start_of(gpu, seeds[0], 7), placed, start_of(gpu, seeds[2], 300)]
    keys = [7, "placed", 300]
    refs = [single_ref(gpu, s, k, st) for s, k, st in zip(seeds, keys, starts)]
    V = refs[1][2]
    lost_at = [int(np.argmax(V[:, k] == OOB)) for k in range(len(xs)) if (V[:, k] == OOB).any()]
    # out of bounds at several frames (table rows), some of them in a later chunk than the first
    assert len(lost_at) >= 4 and len(set(lost_at)) > 3 and max(lost_at) >= CHUNK, lost_at
    assert (refs[1][0][V == OOB] == -1).all() and (refs[1][1][V == OOB] == -1).all()
    d = Dev(gpu)
    got = d.multi([frames_of(gpu, s) for s in seeds], starts)
    d.close()
    for g, r in zip(got, refs):
        same(g, r)


def test_context_state_around_a_multi_call(gpu):
    seqs, starts, refs = selected_case(gpu, COUNTS)
    d = Dev(gpu)
    same(d.single(seqs[0], starts[0]), refs[0])           # plain call first
    for g, r in zip(d.multi(seqs, starts), refs):         # multi after plain
        same(g, r)
    # no current pyramid afterwards: a plain call needs klt_hip_frames_begin
    x = d.up(starts[2][0])
    dfr = d.up(np.stack(seqs[2]))
    assert gpu.klt_hip_track_frames(d.ctx, C.byref(d.pd), C.byref(d.td), dfr + W * H, W, W * H, 1, 1, x, x, x, 0, None,
                                    None, None, 0) == -1
    assert b"klt_hip_frames_begin" in d.error()
    same(d.single(seqs[2], starts[2]), refs[2])           # plain after multi
    same(d.single(seqs[0], starts[0], chunk=64), refs[0])
    for g, r in zip(d.multi(seqs, starts, frame_major=True), refs):
        same(g, r)
    d.close()


def test_refusals_launch_nothing(gpu):
    from kltamd.device import FAST, AffineDesc, TrackDesc
    seqs, starts, _ = selected_case(gpu, COUNTS)
    n = sum(COUNTS)
    d = Dev(gpu)
    d.single(seqs[2], starts[2])
    before = d.kernel()
    assert before and before != MULTI_KERNEL

    def td_with(**kw):
        t = TrackDesc.from_buffer_copy(d.td)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    def refused(what, **kw):
        rc, m, (dx, dy, dv, *_) = d.multi_call(seqs, starts, **kw)
        assert rc == -1, what
        assert d.error(), what
        assert d.kernel() == before, what
        x, y, v = d.down(dx, m, F32), d.down(dy, m, F32), d.down(dv, m, np.int32)
        for got, k in ((x, 0), (y, 1), (v, 2)):
            assert got.tobytes() == np.concatenate([s[k] for s in starts]).tobytes(), what

    ctx = d.ctx
    # configurations
    d.ok(gpu.klt_hip_set_fb(ctx, 1, 0.5), "fb on")
    refused("forward-backward check")
    d.ok(gpu.klt_hip_set_fb(ctx, 0, 0.0), "fb off")
    ad = AffineDesc.from_tc(d.tc.contents)
    ad.mode = 1
    aff, state = d.up(np.zeros(6 * n, F32)), d.up(np.zeros(n, np.int32))
    d.ok(gpu.klt_hip_set_frames_affine(ctx, C.byref(ad), aff, state), "affine on")
    refused("affine check")
    d.ok(gpu.klt_hip_set_frames_affine(ctx, None, None, None), "affine off")
    refused("fast sums", td=td_with(reduction=FAST))
    refused("5x5 window", td=td_with(window_width=5, window_height=5))
    refused("7x9 window", td=td_with(window_height=9))
    refused("lighting-insensitive", td=td_with(lighting_insensitive=1))
    d.ok(gpu.klt_hip_set_path(ctx, 1), "generic pyramids")
    refused("generic pyramid path")
    assert gpu.klt_hip_multi_covers(ctx, C.byref(d.pd), C.byref(d.td)) == 0 and d.error()
    d.ok(gpu.klt_hip_set_path(ctx, 0), "fused pyramids")
    d.ok(gpu.klt_hip_set_track_impl(ctx, 1), "generic tracker")
    refused("generic tracker")
    d.ok(gpu.klt_hip_set_track_impl(ctx, 0), "default tracker")
    # arguments
    refused("nseq 0", nseq=0)
    refused("nseq 65", nseq=65)
    refused("negative count", counts=[300, 0, -1, 9])
    refused("table stride < n", tab_stride=n - 1)
    refused("chunk 0", chunk=0)
    # not even one group of four pyramids per bank
    d.ok(gpu.klt_hip_set_bank_budget(ctx, 2_000_000), "budget")
    refused("bank budget")
    d.ok(gpu.klt_hip_set_bank_budget(ctx, 0), "budget")
    assert gpu.klt_hip_multi_covers(ctx, C.byref(d.pd), C.byref(d.td)) == 1
    d.close()


def _ft_arrays(ft, nfeat, col0, ncol):
    """Columns col0 .. col0+ncol-1 (the ones before are never written: KLTCreateFeatureTable does not clear them)."""
    cell = lambda j, i: ft.contents.feature[j][i].contents  # noqa: E731
    return tuple(np.array([[getattr(cell(j, col0 + i), f) for i in range(ncol)] for j in range(nfeat)], dt)
                 for f, dt in (("x", F32), ("y", F32), ("val", np.int32)))


def _sequences(gpu, seeds, counts, call, tables, ft_col, setup=None):
    """Select on each sequence's frame 0, then `call(tc, arrs, fls, fts)`;
    returns per sequence the final list and the table."""
    from kltabi import fl_affine
    keep = [[np.ascontiguousarray(f) for f in frames_of(gpu, s)] for s in seeds]
    U8P = C.POINTER(C.c_ubyte)
    arrs = [(U8P * (T + 1))(*[u8ptr(f) for f in fr]) for fr in keep]
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    if setup:
        setup(tc.contents)
    fls, fts = [], []
    for fr, n in zip(keep, counts):
        fl = gpu.KLTCreateFeatureList(n)
        gpu.KLTSelectGoodFeatures(tc, u8ptr(fr[0]), W, H, fl)
        fls.append(fl)
        fts.append(gpu.KLTCreateFeatureTable(T + ft_col, n) if tables else None)
    kernel = call(tc, arrs, fls, fts)
    out = []
    for fl, ft, n in zip(fls, fts, counts):
        out.append(fl_to_arrays(fl) + fl_affine(fl) + (_ft_arrays(ft, n, ft_col, T) if ft else ()))
        gpu.KLTFreeFeatureList(fl)
        if ft:
            gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeTrackingContext(tc)
    return out, kernel


def _loop(gpu, ft_col, setup=None):
    def call(tc, arrs, fls, fts):
        for arr, fl, ft in zip(arrs, fls, fts):
            t = gpu.KLTCreateTrackingContext()  # a fresh context per sequence
            t.contents.sequentialMode = 1
            if setup:
                setup(t.contents)
            gpu.KLTTrackSequence(t, arr, T + 1, W, H, fl, ft, ft_col)
            gpu.KLTFreeTrackingContext(t)
        return b""
    return call


def _together(gpu, ft_col):
    def call(tc, arrs, fls, fts):
        from kltamd.abi import FL, FT
        U8PP = C.POINTER(C.POINTER(C.c_ubyte))
        S = len(arrs)
        frames = (U8PP * S)(*[C.cast(a, U8PP) for a in arrs])
        fl = (FL * S)(*fls)
        ft = (FT * S)(*fts) if fts[0] is not None else None
        gpu.KLTTrackSequences(tc, frames, S, T + 1, W, H, fl, ft, ft_col)
        return gpu.klt_hip_track_kernel(gpu.klt_amd_device_context(tc))
    return call


@pytest.mark.parametrize("tables,ft_col", [(False, 0), (True, 0), (True, 2)])
def test_klt_track_sequences_equals_the_loop(gpu, tables, ft_col):
    seeds, counts = SEEDS[:3], [60, 7, 33]
    want, _ = _sequences(gpu, seeds, counts, _loop(gpu, ft_col), tables, ft_col)
    got, kernel = _sequences(gpu, seeds, counts, _together(gpu, ft_col), tables, ft_col)
    assert kernel == MULTI_KERNEL  # tracked together, not by the fallback loop
    assert sum((w[2] == 0).sum() for w in want) > 10
    for g, w in zip(got, want):
        same(g, w)


def test_klt_track_sequences_with_the_affine_check_falls_back(gpu):
    from kltabi import affine_setup
    setup = affine_setup(mode=1)
    seeds, counts = SEEDS[:3], [40, 7, 20]
    want, _ = _sequences(gpu, seeds, counts, _loop(gpu, 1, setup), True, 1, setup)
    got, kernel = _sequences(gpu, seeds, counts, _together(gpu, 1), True, 1, setup)
    assert kernel != MULTI_KERNEL
    for g, w in zip(got, want):
        same(g, w)
