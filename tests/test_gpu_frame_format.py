"""Pyramids and tracking straight from RGB/BGR(A) device frames
(klt_hip_set_frame_format, include/klt_hip.h).

The definition: a colour pixel counts as gray = (4899 R + 9617 G + 1868 B +
8192) >> 14, and whatever is made from a colour frame is, byte for byte, what
the same call makes from that frame converted by the formula.  So every case
compares with the same session's gray call on the frame converted in numpy
(uint32 arithmetic, never the library's own conversion); one tracking case is
held to the oracle as well.

Frames: from a gray synthetic frame f, R = (f >> 1) + 31, G = f, B = lut[f]
with a fixed permutation lut -- three different channels, so reading RGB as
BGR gives another image.

Sizes: 333x251 (odd width: the byte staging path), 320x240 (vectorised:
interior and edge tiles), 160x120 for tracking (tests/test_gpu_multi.py's
shape: 13 tracked frames in chunks of 4), and 256x2064 for the 64-row tiles
that frames of 2000 rows and more take (interior tiles, a ragged last row).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from gpu_helpers import bits
from kltabi import OracleTracker, fl_to_arrays, u8ptr
from kltamd.device import (D2H, FRAME_BGR8, FRAME_BGRA8, FRAME_GRAY8, FRAME_RGB8, FRAME_RGBA8, H2D, PyrDesc,
                           ReplaceDesc, TrackDesc, check)

pytestmark = pytest.mark.gpu

F32 = np.float32
COLOUR = [FRAME_RGB8, FRAME_BGR8, FRAME_RGBA8, FRAME_BGRA8]
BPP = {FRAME_GRAY8: 1, FRAME_RGB8: 3, FRAME_BGR8: 3, FRAME_RGBA8: 4, FRAME_BGRA8: 4}
SIZES = [(333, 251, 333), (320, 240, 240320)]  # w, h, seed
TALL = (256, 2064, 2562064)
W, H, T, CHUNK, N = 160, 120, 13, 4, 300
SEEDS = [160120, 71, 72, 73]
LUT = np.random.default_rng(2024).permutation(256).astype(np.uint8)


def channels(f):
    return ((f >> 1) + 31).astype(np.uint8), f, LUT[f]


def gray_np(r, g, b):
    r, g, b = (np.asarray(c).astype(np.uint32) for c in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def colour(f, fmt, pad=0):
    """The gray frame f as a [H, W * bpp + pad] byte image of `fmt` (alpha: noise)."""
    r, g, b = channels(f)
    h, w = f.shape
    bpp = BPP[fmt]
    px = np.empty((h, w, bpp), np.uint8)
    first, last = (b, r) if fmt in (FRAME_BGR8, FRAME_BGRA8) else (r, b)
    px[..., 0], px[..., 1], px[..., 2] = first, g, last
    if bpp == 4:
        px[..., 3] = np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)
    out = np.full((h, w * bpp + pad), 0xA5, np.uint8)
    out[:, :w * bpp] = px.reshape(h, w * bpp)
    return out


def expected_gray(f):
    return gray_np(*channels(f))


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frames_of(gpu, seed, w=W, h=H, n=T + 1):
    return cached(("frames", seed, w, h, n), lambda: synth(gpu, seed, w, h, n))


def grays_of(gpu, seed):
    return cached(("gray", seed), lambda: [expected_gray(f) for f in frames_of(gpu, seed)])


def start_of(gpu, seed, n, first=None):
    """KLTSelectGoodFeatures (host, gray) on the converted frame 0."""
    def make():
        img = np.ascontiguousarray(grays_of(gpu, seed)[0] if first is None else first)
        if n == 0:
            return np.empty(0, F32), np.empty(0, F32), np.empty(0, np.int32)
        tc = gpu.KLTCreateTrackingContext()
        fl = gpu.KLTCreateFeatureList(n)
        gpu.KLTSelectGoodFeatures(tc, u8ptr(img), img.shape[1], img.shape[0], fl)
        out = fl_to_arrays(fl)
        gpu.KLTFreeFeatureList(fl)
        gpu.KLTFreeTrackingContext(tc)
        return out
    return cached(("start", seed, n), make)


class Dev:
    """A tracking context's device context and the default descriptors for w x h frames."""

    def __init__(self, gpu, w=W, h=H, smooth=1):
        self.gpu, self.w, self.h = gpu, w, h
        self.tc = gpu.KLTCreateTrackingContext()
        self.tc.contents.sequentialMode = 1
        self.ctx = gpu.klt_amd_device_context(self.tc)
        self.pd, self.td = PyrDesc(), TrackDesc()
        gpu.klt_amd_pyr_desc(self.tc, w, h, self.tc.contents.nPyramidLevels, smooth, C.byref(self.pd))
        gpu.klt_amd_track_desc(self.tc, C.byref(self.td))
        self.held = []

    def ok(self, rc, what):
        check(self.gpu, self.ctx, rc, what)

    def fmt(self, f):
        self.ok(self.gpu.klt_hip_set_frame_format(self.ctx, f), "set_frame_format")

    def alloc(self, nbytes):
        d = self.gpu.klt_hip_malloc(self.ctx, max(nbytes, 4))
        assert d
        self.held.append(d)
        return d

    def up(self, a, offset=0):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes + offset) + offset
        if a.nbytes:
            self.ok(self.gpu.klt_hip_memcpy(self.ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        return d

    def down(self, d, shape, dtype):
        a = np.empty(shape, dtype)
        self.ok(self.gpu.klt_hip_sync(self.ctx), "sync")
        if a.nbytes:
            self.ok(self.gpu.klt_hip_memcpy(self.ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return a

    def error(self):
        return self.gpu.klt_hip_last_error(self.ctx).decode()

    def close(self):
        for d in self.held:
            self.gpu.klt_hip_free(self.ctx, d)
        self.gpu.KLTFreeTrackingContext(self.tc)

    # -- pyramids ---------------------------------------------------------
    def pyramid(self, dframe, pitch, fmt, slot=0):
        """klt_hip_build_pyramid from a device frame: the path taken and every level's planes."""
        gpu, ctx = self.gpu, self.ctx
        self.fmt(fmt)
        self.ok(gpu.klt_hip_build_pyramid(ctx, slot, C.byref(self.pd), dframe, pitch, 0), "build")
        self.fmt(FRAME_GRAY8)
        out = []
        for lv in range(self.pd.nlevels):
            w, h = C.c_int(), C.c_int()
            self.ok(gpu.klt_hip_level_dims(ctx, slot, lv, C.byref(w), C.byref(h)), "dims")
            planes = []
            for which in range(3):
                a = np.empty((h.value, w.value), F32)
                self.ok(gpu.klt_hip_download_level(ctx, slot, lv, which, a.ctypes.data), "download")
                planes.append(a)
            out.append(planes)
        return gpu.klt_hip_pyramid_path(ctx, slot), out

    # -- tracking ---------------------------------------------------------
    def lists(self, start, rows=T):
        x, y, v = start
        n = len(x)
        dev = [self.up(a) for a in (x, y, v)]
        tab = [self.up(np.zeros(rows * max(n, 1), F32)) for _ in range(3)]
        return n, dev, tab

    def results(self, n, dev, tab, rows=T):
        return tuple(self.down(d, (rows, n), t) for d, t in zip(tab, (F32, F32, np.int32))) + \
            tuple(self.down(d, n, t) for d, t in zip(dev, (F32, F32, np.int32)))

    def track(self, stack, fmt, start, chunk=CHUNK):
        """klt_hip_frames_begin on stack[0], one klt_hip_track_frames call over
        the rest: the table [T, n] and the final list.  stack: [T + 1, H, pitch] bytes."""
        gpu, ctx = self.gpu, self.ctx
        pitch, stride, t = stack.shape[2], stack.shape[1] * stack.shape[2], stack.shape[0] - 1
        dfr = self.up(stack)
        n, dev, tab = self.lists(start, t)
        self.fmt(fmt)
        self.ok(gpu.klt_hip_frames_begin(ctx, C.byref(self.pd), dfr, pitch), "begin")
        self.ok(gpu.klt_hip_track_frames(ctx, C.byref(self.pd), C.byref(self.td), dfr + stride, pitch, stride, t, chunk,
                                         *dev, n, *tab, n), "track_frames")
        return self.results(n, dev, tab, t)

    def sequence(self, stack, fmt, start):
        """klt_hip_build_pyramid on stack[0], then klt_hip_track_sequence: the final list."""
        gpu, ctx = self.gpu, self.ctx
        pitch, stride = stack.shape[2], stack.shape[1] * stack.shape[2]
        dfr = self.up(stack)
        n, dev, _ = self.lists(start)
        self.fmt(fmt)
        self.ok(gpu.klt_hip_build_pyramid(ctx, 0, C.byref(self.pd), dfr, pitch, 0), "build")
        cur = C.c_int(0)
        self.ok(gpu.klt_hip_track_sequence(ctx, C.byref(self.pd), C.byref(self.td), dfr, pitch, stride, 1, T, *dev, n,
                                           C.byref(cur)), "track_sequence")
        return tuple(self.down(d, n, t) for d, t in zip(dev, (F32, F32, np.int32)))

    def multi(self, stacks, fmt, starts, frame_major):
        """One klt_hip_track_frames_multi call over the sequences' stacks."""
        gpu, ctx = self.gpu, self.ctx
        S = len(stacks)
        pitch = stacks[0].shape[2]
        fb = stacks[0].shape[1] * pitch
        allf = np.stack(stacks)  # [S, T + 1, H, pitch]
        if frame_major:
            allf = np.ascontiguousarray(allf.transpose(1, 0, 2, 3))
            stride, seq_stride = S * fb, fb
        else:
            stride, seq_stride = fb, (T + 1) * fb
        dfr = self.up(allf)
        start = tuple(np.concatenate([s[k] for s in starts]) for k in range(3))
        n, dev, tab = self.lists(start)
        counts = (C.c_int * S)(*[len(s[0]) for s in starts])
        self.fmt(fmt)
        self.ok(gpu.klt_hip_track_frames_multi(ctx, C.byref(self.pd), C.byref(self.td), dfr, pitch, stride, seq_stride,
                                               S, T, CHUNK, counts, *dev, *tab, n), "multi")
        return self.results(n, dev, tab)


def same(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p.shape == q.shape and p.dtype == q.dtype
        assert p.tobytes() == q.tobytes()


def stack_of(gpu, seed, fmt, pad=0):
    if fmt == FRAME_GRAY8:
        return np.stack(grays_of(gpu, seed))
    return np.stack([colour(f, fmt, pad) for f in frames_of(gpu, seed)])


def tracked_pair(gpu, fmt, setup=None, seed=SEEDS[0], how="track"):
    """The same call on the colour frames and on the converted ones, each on a
    context of its own with `setup` applied."""
    out = []
    for f in (fmt, FRAME_GRAY8):
        d = Dev(gpu)
        if setup:
            setup(d)
        out.append(getattr(d, how)(stack_of(gpu, seed, f), f, start_of(gpu, seed, N)))
        d.close()
    return out


# -- 1. klt_hip_to_gray ------------------------------------------------------

@pytest.mark.parametrize("w,h,seed", SIZES)
@pytest.mark.parametrize("fmt", COLOUR)
def test_to_gray(gpu, fmt, w, h, seed):
    fr = frames_of(gpu, seed, w, h, 3)
    src = np.stack([colour(f, fmt, pad=8) for f in fr])  # three frames, padded rows
    d = Dev(gpu, w, h)
    dsrc = d.up(src)
    dpitch = w + 4
    ddst = d.up(np.full((3, h, dpitch), 0x5A, np.uint8))
    d.ok(gpu.klt_hip_to_gray(d.ctx, fmt, dsrc, src.shape[2], src.shape[1] * src.shape[2], 3, w, h, ddst, dpitch,
                             h * dpitch), "to_gray")
    got = d.down(ddst, (3, h, dpitch), np.uint8)
    d.close()
    for k in range(3):
        assert np.array_equal(got[k, :, :w], expected_gray(fr[k]))
    assert (got[:, :, w:] == 0x5A).all()  # dst's padding is not written


# -- 2. the generic path's conversion, directly -----------------------------------

@pytest.mark.parametrize("fmt", [FRAME_RGB8, FRAME_BGRA8])
def test_generic_path_level0_is_the_gray(gpu, fmt):
    w, h, seed = SIZES[0]
    f = frames_of(gpu, seed, w, h, 3)[0]
    d = Dev(gpu, w, h, smooth=0)
    d.ok(gpu.klt_hip_set_path(d.ctx, 1), "set_path")
    src = colour(f, fmt)
    path, lv = d.pyramid(d.up(src), src.shape[1], fmt)
    d.close()
    assert path == 0
    assert np.array_equal(bits(lv[0][0]), bits(expected_gray(f).astype(F32)))


# -- 3. the fused path ----------------------------------------------------------

def fused_case(gpu, w, h, seed, fmt, pad=0, offset=0):
    f = frames_of(gpu, seed, w, h, 3)[0]
    d = Dev(gpu, w, h)
    src = colour(f, fmt, pad)
    path, got = d.pyramid(d.up(src, offset), src.shape[1], fmt, slot=1)
    gpath, want = d.pyramid(d.up(expected_gray(f)), w, FRAME_GRAY8, slot=0)
    d.close()
    assert path == 1 and gpath == 1
    assert len(got) == len(want) == 2
    for lg, lw in zip(got, want):
        for pg, pw in zip(lg, lw):
            assert pg.shape == pw.shape and np.array_equal(bits(pg), bits(pw))
    assert np.abs(want[0][1]).max() > 1 and np.abs(want[1][2]).max() > 1  # real gradients on both levels


@pytest.mark.parametrize("w,h,seed", SIZES)
@pytest.mark.parametrize("fmt", COLOUR)
def test_fused_pyramid(gpu, fmt, w, h, seed):
    fused_case(gpu, w, h, seed, fmt)


@pytest.mark.parametrize("pad,offset", [(12, 0), (0, 4), (0, 1)], ids=["pitch+12", "base+4", "base+1-bytes"])
def test_fused_pyramid_pitch_and_base(gpu, pad, offset):
    w, h, seed = SIZES[1]
    fused_case(gpu, w, h, seed, FRAME_RGB8, pad, offset)


@pytest.mark.parametrize("fmt", [FRAME_RGB8, FRAME_BGRA8])
def test_fused_pyramid_tall(gpu, fmt):
    fused_case(gpu, *TALL, fmt)


# -- 4. batched tracking ----------------------------------------------------------

def gray_run(gpu, lazy, sched):
    def make():
        d = Dev(gpu)
        d.ok(gpu.klt_hip_set_lazy_grad(d.ctx, lazy), "lazy")
        d.ok(gpu.klt_hip_set_frames_overlap(d.ctx, sched), "sched")
        out = d.track(stack_of(gpu, SEEDS[0], FRAME_GRAY8), FRAME_GRAY8, start_of(gpu, SEEDS[0], N))
        d.close()
        return out
    return cached(("gray_run", lazy, sched), make)


@pytest.mark.parametrize("lazy,sched", [(1, 0), (0, 0), (1, 3)], ids=["lazy", "records", "lazy-tail"])
@pytest.mark.parametrize("fmt", [FRAME_RGB8, FRAME_BGRA8])
def test_track_frames(gpu, oracle, fmt, lazy, sched):
    want = gray_run(gpu, lazy, sched)
    assert (want[2][-1] == 0).sum() > 10  # the case is real: features survive the sequence
    d = Dev(gpu)
    d.ok(gpu.klt_hip_set_lazy_grad(d.ctx, lazy), "lazy")
    d.ok(gpu.klt_hip_set_frames_overlap(d.ctx, sched), "sched")
    got = d.track(stack_of(gpu, SEEDS[0], fmt), fmt, start_of(gpu, SEEDS[0], N))
    d.close()
    same(got, want)
    if fmt == FRAME_RGB8:
        g = grays_of(gpu, SEEDS[0])
        OX, OY, OV = cached("oracle", lambda: OracleTracker(oracle).harness(g, N, T + 1, first=g[0]))
        X, Y, V = got[:3]
        for j in range(T):
            assert np.array_equal(V[j], OV[:, j])
            assert np.array_equal(bits(X[j]), bits(OX[:, j])) and np.array_equal(bits(Y[j]), bits(OY[:, j]))


def layout_setup(gpu, layout):
    """The three level-0 layouts of a bank: the image plane alone (lazy
    gradients), records, and the planes the generic tracker reads."""
    def setup(d):
        d.ok(gpu.klt_hip_set_lazy_grad(d.ctx, 1 if layout == "image" else 0), "lazy")
        d.ok(gpu.klt_hip_set_track_impl(d.ctx, 1 if layout == "planes" else 0), "impl")
    return setup


def test_track_frames_planes(gpu):
    got, want = tracked_pair(gpu, FRAME_RGB8, layout_setup(gpu, "planes"))
    same(got, want)
    same(want, gray_run(gpu, 1, 0))


@pytest.mark.parametrize("layout", ["image", "records", "planes"])
def test_track_frames_tall(gpu, layout):
    """Two tracked frames of 2064 rows: the 64-row instances of every layout."""
    w, h, seed = TALL
    fr = frames_of(gpu, seed, w, h, 3)
    start = start_of(gpu, seed, 64, first=expected_gray(fr[0]))
    out = []
    for f in (FRAME_RGB8, FRAME_GRAY8):
        stack = np.stack([expected_gray(a) if f == FRAME_GRAY8 else colour(a, f) for a in fr])
        d = Dev(gpu, w, h)
        layout_setup(gpu, layout)(d)
        out.append(d.track(stack, f, start, chunk=2))
        d.close()
    same(*out)
    assert (out[1][2][-1] == 0).sum() > 10


# -- 5. composition -----------------------------------------------------------------

@pytest.mark.parametrize("frame_major", [False, True])
def test_multi(gpu, frame_major):
    counts = [300, 0, 7, 1]
    starts = [start_of(gpu, s, n) for s, n in zip(SEEDS, counts)]
    out = []
    for f in (FRAME_RGB8, FRAME_GRAY8):
        d = Dev(gpu)
        out.append(d.multi([stack_of(gpu, s, f) for s in SEEDS], f, starts, frame_major))
        d.close()
    same(*out)
    assert (out[1][2][-1][:300] == 0).sum() > 10


def test_forward_backward(gpu):
    got, want = tracked_pair(gpu, FRAME_RGB8, lambda d: d.ok(gpu.klt_hip_set_fb(d.ctx, 1, 0.05), "fb"))
    same(got, want)
    assert (want[2][-1] == 0).sum() > 10


def test_replacement_inside_the_call(gpu):
    def setup(d):
        rd = ReplaceDesc.from_tc(d.tc.contents, 2)
        d.ok(gpu.klt_hip_set_frames_replace(d.ctx, C.byref(rd)), "replace")
    got, want = tracked_pair(gpu, FRAME_RGB8, setup)
    same(got, want)
    assert (want[2][-1] >= 0).sum() > 10


def test_track_sequence(gpu):
    got, want = tracked_pair(gpu, FRAME_RGB8, how="sequence")
    same(got, want)
    assert (want[2] == 0).sum() > 10
    same(want, gray_run(gpu, 1, 0)[3:])  # and the batched call's final list


# -- 6. channel order ---------------------------------------------------------------

def test_channel_order_matters(gpu):
    rgb = stack_of(gpu, SEEDS[0], FRAME_RGB8)
    a, b = (expected_gray(frames_of(gpu, SEEDS[0])[0]), gray_np(*channels(frames_of(gpu, SEEDS[0])[0])[::-1]))
    assert (a != b).mean() > 0.99
    out = []
    for f in (FRAME_RGB8, FRAME_BGR8):
        d = Dev(gpu)
        out.append(d.track(rgb, f, start_of(gpu, SEEDS[0], N)))
        d.close()
    same(out[0], gray_run(gpu, 1, 0))
    assert out[0][3].tobytes() != out[1][3].tobytes() or out[0][4].tobytes() != out[1][4].tobytes()


# -- 7. the setting and the refusals ---------------------------------------------------

def test_setting(gpu):
    d = Dev(gpu)
    ctx = d.ctx
    assert gpu.klt_hip_get_frame_format(ctx) == FRAME_GRAY8
    for f in COLOUR + [FRAME_GRAY8, FRAME_RGBA8]:
        assert gpu.klt_hip_set_frame_format(ctx, f) == 0 and gpu.klt_hip_get_frame_format(ctx) == f
    for bad in (-1, 5):
        assert gpu.klt_hip_set_frame_format(ctx, bad) == -1
        assert "format" in d.error() and gpu.klt_hip_get_frame_format(ctx) == FRAME_RGBA8
    d.ok(gpu.klt_hip_ctx_reset(ctx), "reset")
    assert gpu.klt_hip_get_frame_format(ctx) == FRAME_GRAY8
    d.close()


def test_refusals(gpu):
    seed = SEEDS[0]
    start = start_of(gpu, seed, N)
    rgb, gray = stack_of(gpu, seed, FRAME_RGB8), stack_of(gpu, seed, FRAME_GRAY8)
    d = Dev(gpu)
    ctx, pd, td = d.ctx, C.byref(d.pd), C.byref(d.td)
    drgb, dgray = d.up(rgb), d.up(gray)
    n, dev, _ = d.lists(start)
    esc = d.up(np.zeros(1, np.int32))

    def untouched(rc, word, kernel):
        assert rc == -1
        assert word in d.error(), d.error()
        assert gpu.klt_hip_track_kernel(ctx) == kernel
        for dd, a in zip(dev, start):
            assert d.down(dd, a.shape, a.dtype).tobytes() == a.tobytes()

    d.fmt(FRAME_RGB8)
    d.ok(gpu.klt_hip_frames_begin(ctx, pd, drgb, 3 * W), "begin")
    kernel = gpu.klt_hip_track_kernel(ctx)
    assert gpu.klt_hip_frames_begin(ctx, pd, drgb, 3 * W - 1) == -1 and "pitch" in d.error()
    assert gpu.klt_hip_build_pyramid(ctx, 0, pd, drgb, 3 * W - 1, 0) == -1 and "pitch" in d.error()
    untouched(gpu.klt_hip_track_frames(ctx, pd, td, drgb + 3 * W * H, 3 * W - 1, 3 * W * H, T, CHUNK, *dev, n, None,
                                       None, None, 0), "pitch", kernel)
    counts = (C.c_int * 1)(n)
    untouched(gpu.klt_hip_track_frames_multi(ctx, pd, td, drgb, 3 * W - 1, 3 * W * H, 3 * W * H * (T + 1), 1, T, CHUNK,
                                             counts, *dev, None, None, None, 0), "pitch", kernel)

    def band(frames, pitch):
        return gpu.klt_hip_track_frames_band(ctx, pd, td, frames + pitch * H, pitch, pitch * H, 3, *dev, n,
                                             float("-inf"), float("inf"), 0, H, esc, None, 0)
    untouched(band(drgb, 3 * W), "colour", kernel)
    # gray again: the band call works, from the converted frames
    d.fmt(FRAME_GRAY8)
    d.ok(gpu.klt_hip_frames_begin(ctx, pd, dgray, W), "begin")
    d.ok(band(dgray, W), "band")
    banded = tuple(d.down(dd, a.shape, a.dtype) for dd, a in zip(dev, start))
    d.close()
    want = gray_run(gpu, 1, 0)
    assert banded[2].tobytes() == want[2][2].tobytes()  # the statuses after three frames
    assert banded[0].tobytes() == want[0][2].tobytes() and banded[1].tobytes() == want[1][2].tobytes()


def test_sharded_driver_refuses_colour(gpu):
    """klt_shard_track and klt_shard_eigen: refused before any launch, the arrays untouched.
    (A one-rank local shard; most of this test's seconds are the process's first
    communicator, which tests/test_shard.py otherwise pays.)"""
    from kltamd.device import SelectDesc
    seed = SEEDS[0]
    start = start_of(gpu, seed, N)
    d = Dev(gpu)
    drgb = d.up(stack_of(gpu, seed, FRAME_RGB8))
    n, dev, _ = d.lists(start)
    s = gpu.klt_shard_create_local(d.ctx, 0, 1, H, 32)
    assert s, gpu.klt_shard_create_error()
    d.fmt(FRAME_RGB8)
    d.ok(gpu.klt_hip_frames_begin(d.ctx, C.byref(d.pd), drgb, 3 * W), "begin")
    kernel = gpu.klt_hip_track_kernel(d.ctx)
    rc = gpu.klt_shard_track(s, C.byref(d.pd), C.byref(d.td), drgb + 3 * W * H, 3 * W, 3 * W * H, 3, None, 0, *dev, n,
                             None, None)
    assert rc < 0 and b"colour" in gpu.klt_shard_last_error(s)
    t = d.tc.contents
    sd = SelectDesc(t.window_width, t.window_height, max(t.borderx, t.window_width // 2),
                    max(t.bordery, t.window_height // 2), t.nSkippedPixels)
    emap = d.alloc(4 * W * H)
    rc = gpu.klt_shard_eigen(s, C.byref(d.pd), C.byref(sd), 3 * W, emap, None, None)
    assert rc < 0 and b"colour" in gpu.klt_shard_last_error(s)
    assert gpu.klt_hip_track_kernel(d.ctx) == kernel
    for dd, a in zip(dev, start):
        assert d.down(dd, a.shape, a.dtype).tobytes() == a.tobytes()
    gpu.klt_shard_destroy(s)
    d.close()


def test_host_frames_stay_gray(gpu):
    seed = SEEDS[0]
    x, y, v = (a.copy() for a in start_of(gpu, seed, N))
    keep = [np.ascontiguousarray(f) for f in grays_of(gpu, seed)]
    arr = (C.POINTER(C.c_ubyte) * len(keep))(*[u8ptr(f) for f in keep])
    d = Dev(gpu)
    d.fmt(FRAME_RGB8)
    d.ok(gpu.klt_hip_track_frames_host(d.ctx, C.byref(d.pd), C.byref(d.td), arr, len(keep), 1, CHUNK, x.ctypes.data,
                                       y.ctypes.data, v.ctypes.data, N, None, None), "track_frames_host")
    assert gpu.klt_hip_get_frame_format(d.ctx) == FRAME_RGB8  # the setting itself is kept
    d.close()
    same((x, y, v), gray_run(gpu, 1, 0)[3:])
