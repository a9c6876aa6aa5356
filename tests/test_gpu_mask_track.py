"""The region mask's tracking use on the GPU (klt_hip_set_mask with
KLT_HIP_MASK_TRACK) against its CPU statement (tests/native/mask_oracle.c
through mask_scenes.shim_table): x, y and val bit for bit, table rows included,
on every call that honours the setting, with klt_hip_set_track_merge 0/1,
klt_hip_set_lazy_grad 0/1 and input / band order; every call that refuses it;
and, with the selection use alone, the forward-backward check and the
multi-sequence replacement."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import mask_scenes as ms
from motion_scenes import F32, H, MAX_ITERATIONS, W, placed_list, scene
from test_mask_host import bits

pytestmark = pytest.mark.gpu

T = ms.T
KERNEL = b"kltdev::k_track7_mask<true, 2>"            # full level-0 records: per-call tracking, klt_hip_set_lazy_grad 0
LAZY_MASK = b"kltdev::k_track7_mask_lazy<2>"           # the batched calls' image-only level 0
LAZY_KERNEL = b"kltdev::k_track7<false, true, 2, false, true>"
HOOKS = list(itertools.product((0, 1), (0, 1), (0, 1)))  # track_merge, lazy_grad, input order


def assert_rows_equal(got, want, names="x y val"):
    for g, w, name in zip(got, want, names.split()):
        assert g.shape == w.shape, name
        bad = np.argwhere(bits(g) != bits(w))
        assert not len(bad), f"{name} differs first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


class Dev:
    """One device context with the scene's frames, a list, tables and masks in device memory."""

    def __init__(self, gpu, frames, start, mask=None, flags=ms.MASK_TRACK, setup=None):
        from kltamd.device import PyrDesc, TrackDesc, check
        self.gpu, self.check = gpu, check
        self.start = start
        self.n = n = len(start[0])
        self.tc = tc = gpu.KLTCreateTrackingContext()
        tc.contents.sequentialMode = 1
        if setup:
            setup(tc.contents)
        self.ctx = gpu.klt_amd_device_context(tc)
        self.nbuf = []
        stack = np.ascontiguousarray(np.stack(frames))
        self.dfr = self.up(stack)
        self.list = [self.up(np.ascontiguousarray(a)) for a in start]
        self.tabs = [self.up(np.full((T, n), 7.0, F32)) for _ in range(3)]
        self.pd, self.td = PyrDesc(), TrackDesc()
        gpu.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(self.pd))
        gpu.klt_amd_track_desc(tc, C.byref(self.td))
        self.dmask = None
        if mask is not None:
            self.set_mask(mask, flags)

    def up(self, a):
        d = self.gpu.klt_hip_malloc(self.ctx, max(a.nbytes, 1))
        assert d
        self.nbuf.append(d)
        self.put(d, a)
        return d

    def put(self, d, a):
        from kltamd.device import H2D
        a = np.ascontiguousarray(a)
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_memcpy(self.ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")

    def get(self, d, shape, dtype):
        from kltamd.device import D2H
        a = np.empty(shape, dtype)
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_sync(self.ctx), "sync")
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_memcpy(self.ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return a

    def set_mask(self, mask, flags=ms.MASK_TRACK):
        self.dmask = self.up(mask)
        assert self.gpu.klt_hip_set_mask(self.ctx, self.dmask, mask.shape[1], flags) == 0

    def hooks(self, merge, lazy, order):
        g = self.gpu
        assert g.klt_hip_set_track_merge(self.ctx, merge) == 0 and g.klt_hip_set_lazy_grad(self.ctx, lazy) == 0
        assert g.klt_hip_set_track_order(self.ctx, order) == 0

    def reset_lists(self, start=None):
        for d, a in zip(self.list, start or self.start):
            self.put(d, a)
        for d in self.tabs:
            self.put(d, np.full((T, self.n), 7.0, F32))

    def frame(self, i):
        return self.dfr + i * W * H

    def pyramid(self, slot, i):
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_build_pyramid(self.ctx, slot, C.byref(self.pd), self.frame(i), W, 0),
                   "pyramid")

    def begin(self, i=0):
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_frames_begin(self.ctx, C.byref(self.pd), self.frame(i), W), "begin")

    def track_frames(self, j0, nf, chunk, tables=True, td=None):
        n, off = self.n, 4 * self.n * j0
        tx, ty, tv = (t + off if tables else None for t in self.tabs)
        return self.gpu.klt_hip_track_frames(self.ctx, C.byref(self.pd), C.byref(td or self.td), self.frame(1 + j0), W, W * H,
                                             nf, chunk, *self.list, n, tx, ty, tv, n)

    def lists(self):
        return tuple(self.get(d, self.n, np.int32 if k == 2 else F32) for k, d in enumerate(self.list))

    def tables(self):
        return tuple(self.get(d, (T, self.n), np.int32 if k == 2 else F32) for k, d in enumerate(self.tabs))

    def list_bytes(self):
        return b"".join(a.tobytes() for a in self.lists())

    def kernel(self):
        return self.gpu.klt_hip_track_kernel(self.ctx)

    def error(self):
        m = self.gpu.klt_hip_last_error(self.ctx)
        return m.decode() if m else ""

    def close(self):
        g = self.gpu
        g.klt_hip_sync(self.ctx)
        g.klt_hip_set_mask(self.ctx, None, 0, 0)
        g.klt_hip_set_frames_replace(self.ctx, None)
        g.klt_hip_set_fb(self.ctx, 0, 0.0)
        for d in self.nbuf:
            g.klt_hip_free(self.ctx, d)
        g.KLTFreeTrackingContext(self.tc)


@pytest.fixture
def dev(gpu):
    made = []

    def make(frames, start, **kw):
        made.append(Dev(gpu, frames, start, **kw))
        return made[-1]
    yield make
    for d in made:
        d.close()


def want_placed(seed):
    ms.assert_scene_conditions(seed)  # before any comparison
    return ms.placed_table(seed)[:3]


# ---------------------------------------------------------------------------
# the calls that honour the setting
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SEEDS)
def test_per_call_track_loop(gpu, dev, seed):
    want = want_placed(seed)
    d = dev(scene(seed), placed_list(), mask=ms.scene_mask())
    g = d.gpu
    for merge, lazy, order in HOOKS:
        d.hooks(merge, lazy, order)
        d.reset_lists()
        rows = []
        d.pyramid(0, 0)
        for i in range(1, T + 1):
            s1, s2 = (i - 1) % 2, i % 2
            d.pyramid(s2, i)
            d.check(g, d.ctx, g.klt_hip_track(d.ctx, s1, s2, C.byref(d.td), *d.list, d.n, 1), "track")
            assert d.kernel() == KERNEL
            rows.append(d.lists())
        assert_rows_equal(tuple(np.stack([r[k] for r in rows]) for k in range(3)), want)


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_track_sequence_steps(gpu, dev, seed):
    want = want_placed(seed)
    d = dev(scene(seed), placed_list(), mask=ms.scene_mask())
    g = d.gpu
    for merge, lazy, order in HOOKS:
        d.hooks(merge, lazy, order)
        d.reset_lists()
        d.pyramid(0, 0)
        cur = C.c_int(0)
        d.check(g, d.ctx, g.klt_hip_track_sequence(d.ctx, C.byref(d.pd), C.byref(d.td), d.dfr, W, W * H, 1, T, *d.list, d.n,
                                                   C.byref(cur)), "track_sequence")
        assert d.kernel() == KERNEL
        assert_rows_equal(d.lists(), tuple(w[-1] for w in want))


@pytest.mark.parametrize("seed", ms.SEEDS)
@pytest.mark.parametrize("chunk", [4, 13])
def test_track_frames_chunks(gpu, dev, seed, chunk):
    """Chunks of 4: the last one is ragged."""
    want = want_placed(seed)
    d = dev(scene(seed), placed_list(), mask=ms.scene_mask())
    for merge, lazy, order in HOOKS:
        d.hooks(merge, lazy, order)
        d.reset_lists()
        d.begin()
        d.check(d.gpu, d.ctx, d.track_frames(0, T, chunk), "frames")
        assert d.kernel() == (LAZY_MASK if lazy else KERNEL)
        assert_rows_equal(d.tables(), want)
        assert_rows_equal(d.lists(), tuple(w[-1] for w in want))


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_one_call_equals_two(gpu, dev, seed):
    want = want_placed(seed)
    d = dev(scene(seed), placed_list(), mask=ms.scene_mask())
    d.begin()
    d.check(d.gpu, d.ctx, d.track_frames(0, 6, 4), "frames")
    assert_rows_equal(d.lists(), tuple(w[5] for w in want))
    d.check(d.gpu, d.ctx, d.track_frames(6, 7, 4), "frames")
    assert_rows_equal(d.tables(), want)


_ROWS = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                    C.POINTER(C.c_int), C.c_long)


def frames_host(gpu, d, frames, start, chunk=4):
    n = len(start[0])
    x, y, v = (a.copy() for a in start)
    X, Y, V = np.zeros((T, n), F32), np.zeros((T, n), F32), np.zeros((T, n), np.int32)

    def rows(user, frame0, nframes, f0, f1, rx, ry, rv, stride):
        for j in range(nframes):
            for dst, src in ((X, rx), (Y, ry), (V, rv)):
                dst[frame0 + j, f0:f1] = np.ctypeslib.as_array(src, shape=((j + 1) * stride,))[j * stride + f0:j * stride + f1]

    cb = _ROWS(rows)
    arr = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    rc = gpu.klt_hip_track_frames_host(d.ctx, C.byref(d.pd), C.byref(d.td), arr, len(frames), 1, chunk, x.ctypes.data,
                                       y.ctypes.data, v.ctypes.data, n, cb, None)
    return rc, (X, Y, V), (x, y, v)


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_track_frames_host(gpu, dev, seed):
    want = want_placed(seed)
    frames = [np.ascontiguousarray(f) for f in scene(seed)]
    d = dev(frames, placed_list(), mask=ms.scene_mask())
    for merge, lazy, order in HOOKS:
        d.hooks(merge, lazy, order)
        rc, tab, lst = frames_host(gpu, d, frames, placed_list())
        d.check(gpu, d.ctx, rc, "frames_host")
        assert d.kernel() == (LAZY_MASK if lazy else KERNEL)
        assert_rows_equal(tab, want)
        assert_rows_equal(lst, tuple(w[-1] for w in want))


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_max_iterations_precedence(gpu, dev, seed):
    """The mask beats KLT_MAX_ITERATIONS: the case mask_scenes.maxit_table makes."""
    mask, want, (row, k) = ms.maxit_table(seed)
    assert want[2][row, k] == ms.MASKED and want[3][row, k] == MAX_ITERATIONS  # on the shim first
    d = dev(scene(seed), placed_list(), mask=mask)
    for merge in (0, 1):
        d.hooks(merge, 1, 0)
        d.reset_lists()
        d.begin()
        d.check(d.gpu, d.ctx, d.track_frames(0, T, 4), "frames")
        tab = d.tables()
        assert_rows_equal(tab, want[:3])
        assert tab[2][row, k] == ms.MASKED


@pytest.mark.parametrize("seed", ms.SEEDS)
@pytest.mark.parametrize("pad", [0, 1])
def test_pitch_wider_than_the_image(gpu, dev, seed, pad):
    want = want_placed(seed)
    d = dev(scene(seed), placed_list(), mask=ms.scene_mask(pitch=W + 37, pad=pad))
    d.begin()
    d.check(d.gpu, d.ctx, d.track_frames(0, T, 4), "frames")
    assert_rows_equal(d.tables(), want)


@pytest.mark.parametrize("seed", ms.SEEDS)
@pytest.mark.parametrize("chunk", [4, 13])
@pytest.mark.parametrize("host", [False, True])
def test_replacement_inside_the_call(gpu, dev, seed, chunk, host):
    """klt_hip_set_frames_replace every 3 frames with both bits set, against the
    shim's loop: orc_track_mask, then orc_replace_mask."""
    from kltamd.device import ReplaceDesc
    mask = ms.scene_mask()
    want = ms.shim_table(("replace", seed), scene(seed), placed_list(), track_mask=mask, select_mask=mask, every=3)
    V, X, Y = want[2], want[0], want[1]
    # on the shim first: slots are refilled, never on a masked pixel, and features are lost to the mask
    refilled = [(j, (V[j] > 0)) for j in (2, 5, 8, 11)]
    assert sum(int(f.sum()) for _, f in refilled) >= 20
    for j, f in refilled:
        assert (mask[Y[j][f].astype(int), X[j][f].astype(int)] != 0).all()
    assert (V == ms.MASKED).sum() >= ms.FLOORS["masked"]
    frames = [np.ascontiguousarray(f) for f in scene(seed)]
    d = dev(frames, placed_list(), mask=mask, flags=ms.MASK_TRACK | ms.MASK_SELECT)
    rd = ReplaceDesc.from_tc(d.tc.contents, 3)
    for merge, lazy in ((1, 1), (0, 0)):
        d.hooks(merge, lazy, 0)
        d.reset_lists()
        assert gpu.klt_hip_set_frames_replace(d.ctx, C.byref(rd)) == 0
        if host:
            rc, tab, lst = frames_host(gpu, d, frames, placed_list(), chunk)
        else:
            d.begin()
            rc = d.track_frames(0, T, chunk)
        assert gpu.klt_hip_set_frames_replace(d.ctx, None) == 0
        d.check(gpu, d.ctx, rc, "frames")
        if not host:
            tab, lst = d.tables(), d.lists()
        assert_rows_equal(tab, want[:3])
        assert_rows_equal(lst, tuple(w[-1] for w in want[:3]))


# ---------------------------------------------------------------------------
# all allowed / off: today's bytes and kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SEEDS)
def test_all_allowed_gives_the_bytes_of_no_mask(gpu, dev, seed):
    want = ms.placed_table(seed, masked=False)[:3]
    d = dev(scene(seed), placed_list())
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, T, 4), "frames")
    none = d.tables()
    assert_rows_equal(none, want)
    d.set_mask(np.ones((H, W), np.uint8))
    d.reset_lists()
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, T, 4), "frames")
    assert d.kernel() == LAZY_MASK
    assert_rows_equal(d.tables(), none)
    assert gpu.klt_hip_set_lazy_grad(d.ctx, 0) == 0
    d.reset_lists()
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, T, 4), "frames")
    assert d.kernel() == KERNEL
    assert_rows_equal(d.tables(), none)


def test_setting_off_keeps_the_kernel(gpu, dev):
    fr = scene(7)[:3]
    d = dev(fr, placed_list())

    def run():
        d.reset_lists()
        d.begin()
        d.check(gpu, d.ctx, d.track_frames(0, 2, 2), "frames")
        return d.kernel()

    assert run() == LAZY_KERNEL
    d.set_mask(ms.scene_mask(), ms.MASK_SELECT)  # the selection use alone: the tracker of before
    assert run() == LAZY_KERNEL
    d.set_mask(ms.scene_mask(), ms.MASK_TRACK)
    assert run() == LAZY_MASK
    assert gpu.klt_hip_set_lazy_grad(d.ctx, 0) == 0
    assert run() == KERNEL
    assert gpu.klt_hip_set_lazy_grad(d.ctx, 1) == 0
    assert gpu.klt_hip_set_mask(d.ctx, None, 0, 0) == 0
    assert run() == LAZY_KERNEL
    d.set_mask(ms.scene_mask(), ms.MASK_TRACK | ms.MASK_SELECT)
    assert run() == LAZY_MASK
    assert gpu.klt_hip_set_mask(d.ctx, d.dmask, W, 0) == 0  # flags 0 clears it
    flags = C.c_int(9)
    assert gpu.klt_hip_get_mask(d.ctx, None, None, C.byref(flags)) == 0 and flags.value == 0
    d.set_mask(ms.scene_mask(), ms.MASK_TRACK)
    assert gpu.klt_hip_ctx_reset(d.ctx) == 0  # ... and so does a reset
    assert gpu.klt_hip_get_mask(d.ctx, None, None, C.byref(flags)) == 0 and flags.value == 0
    assert run() == LAZY_KERNEL


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu, dev):
    """-1 and a message naming the setting, before any launch: x, y and val
    byte for byte as they were."""
    from kltamd.device import FAST, AffineDesc, ReplaceDesc, TrackDesc
    fr = scene(7)[:4]
    d = dev(fr, placed_list(), mask=ms.scene_mask())
    g, ctx, n = gpu, d.ctx, d.n
    d.begin()
    before = d.list_bytes()
    x, y, v = d.list

    def td(**kw):
        t = TrackDesc.from_buffer_copy(d.td)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    def frames(t=None):
        return d.track_frames(0, 3, 2, tables=False, td=t)

    def refused(rc, what):
        assert rc == -1, what
        assert "klt_hip_set_mask" in d.error(), (what, d.error())
        assert d.list_bytes() == before, what

    # the forward-backward check, the affine check, the motion prior, fast sums
    assert g.klt_hip_set_fb(ctx, 1, 1.0) == 0
    refused(frames(), "fb")
    assert g.klt_hip_set_fb(ctx, 0, 0.0) == 0
    ad = AffineDesc(0, 15, 15, 10, 0.01, 0.1, 0.02, 10.0, 1.5, 1.0, 0)
    scratch = d.up(np.zeros(6 * n, F32))
    assert g.klt_hip_affine_reserve(ctx, n, 15, 15) >= 0
    assert g.klt_hip_set_frames_affine(ctx, C.byref(ad), scratch, scratch) == 0
    refused(frames(), "affine inside the launch")
    assert g.klt_hip_set_frames_affine(ctx, None, None, None) == 0
    vx, vy = d.up(np.zeros(n, F32)), d.up(np.zeros(n, F32))
    assert g.klt_hip_set_predict(ctx, 1, vx, vy) == 0
    refused(frames(), "motion prior")
    assert g.klt_hip_set_predict(ctx, 0, None, None) == 0
    refused(frames(td(reduction=FAST)), "fast sums")
    # the generic tracker: other windows, lighting-insensitive mode, forced
    refused(frames(td(window_width=9, window_height=9)), "window 9")
    refused(frames(td(lighting_insensitive=1)), "lighting-insensitive")
    assert g.klt_hip_set_track_impl(ctx, 1) == 0
    refused(frames(), "generic kernel")
    assert g.klt_hip_set_track_impl(ctx, 0) == 0
    # band calls and the sharded driver
    esc = d.up(np.zeros(1, np.int32))
    refused(g.klt_hip_track_frames_band(ctx, C.byref(d.pd), C.byref(d.td), d.frame(1), W, W * H, 2, x, y, v, n, 0.0,
                                        float(H), 0, H, esc, None, 0), "band")
    s = g.klt_shard_create_local(ctx, 0, 1, H, 16)
    assert s, g.klt_shard_create_error()
    rc = g.klt_shard_track(s, C.byref(d.pd), C.byref(d.td), d.frame(1), W, W * H, 2, None, 0, x, y, v, n, None, None)
    msg = g.klt_shard_last_error(s).decode()
    g.klt_shard_destroy(s)
    assert rc < 0 and "klt_hip_set_mask" in msg and d.list_bytes() == before
    # the multi-sequence calls
    counts = (C.c_int * 1)(n)
    refused(g.klt_hip_multi_covers(ctx, C.byref(d.pd), C.byref(d.td)), "multi_covers")
    refused(g.klt_hip_track_frames_multi(ctx, C.byref(d.pd), C.byref(d.td), d.dfr, W, W * H, W * H, 1, 2, 2, counts, x, y,
                                         v, None, None, None, 0), "multi")
    rd = ReplaceDesc.from_tc(d.tc.contents, 2)
    refused(g.klt_hip_track_frames_multi_replace(ctx, C.byref(d.pd), C.byref(d.td), C.byref(rd), 0, d.dfr, W, W * H,
                                                 W * H, 1, 2, 2, counts, x, y, v, None, None, None, 0, None, None, None),
            "multi_replace")
    # klt_hip_track with host arrays, klt_hip_track_affine
    for slot in (0, 1):
        d.pyramid(slot, slot)
    hx, hy, hv = (a.copy() for a in placed_list())
    hb = hx.tobytes() + hy.tobytes() + hv.tobytes()
    refused(g.klt_hip_track(ctx, 0, 1, C.byref(d.td), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data, n, 0), "host arrays")
    assert hx.tobytes() + hy.tobytes() + hv.tobytes() == hb
    aff, st = np.zeros((n, 6), F32), np.zeros(n, np.int32)
    fn = g.klt_hip_track_affine  # another module may have bound its own pointer types: cast to whatever they are
    ptrs = [C.cast(p, t) for p, t in zip((C.pointer(d.td), C.pointer(ad), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data,
                                          aff.ctypes.data, st.ctypes.data), fn.argtypes[3:10])]
    refused(fn(ctx, 0, 1, *ptrs, n), "track_affine")
    assert hx.tobytes() + hy.tobytes() + hv.tobytes() == hb
    # a pitch below the image's width
    assert g.klt_hip_set_mask(ctx, d.dmask, W - 1, ms.MASK_TRACK) == 0
    refused(frames(), "pitch")
    refused(g.klt_hip_track(ctx, 0, 1, C.byref(d.td), x, y, v, n, 1), "pitch, per call")
    cur = C.c_int(0)
    refused(g.klt_hip_track_sequence(ctx, C.byref(d.pd), C.byref(d.td), d.dfr, W, W * H, 1, 2, x, y, v, n, C.byref(cur)),
            "pitch, track_sequence")
    # flags outside the two bits leave the setting as it is
    assert g.klt_hip_set_mask(ctx, d.dmask, W, 7) == -1
    p, pitch, flags = C.c_void_p(), C.c_long(), C.c_int()
    assert g.klt_hip_get_mask(ctx, C.byref(p), C.byref(pitch), C.byref(flags)) == 0
    assert (p.value, pitch.value, flags.value) == (d.dmask, W - 1, ms.MASK_TRACK)
    # ... and the call it covers runs
    assert g.klt_hip_set_mask(ctx, d.dmask, W, ms.MASK_TRACK) == 0
    d.begin()
    d.check(g, ctx, frames(), "frames")
    want = ms.placed_table(7)
    assert_rows_equal(d.lists(), tuple(w[2] for w in want[:3]))


# ---------------------------------------------------------------------------
# the selection use alone refuses nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SEEDS)
def test_selection_bit_with_the_forward_backward_check(gpu, dev, seed):
    """FB on, replacement every 3 frames inside the call, the mask's selection
    use: the shim's forward and backward steps, test_fb's verdict, then
    orc_replace_mask."""
    from kltamd.device import ReplaceDesc
    from test_fb import FB_REJECTED, fb_verdict
    fr, mask, dist = scene(seed), ms.scene_mask(), 0.5
    f, b = ms.Shim(), ms.Shim(sequential=0)
    x, y, v = (a.copy() for a in placed_list())
    rows = []
    for i in range(1, T + 1):
        x0, y0 = x.copy(), y.copy()
        f.track_mask(fr[i - 1], fr[i], x, y, v, None)
        xb, yb, vb = x.copy(), y.copy(), v.copy()
        b.track(fr[i], fr[i - 1], xb, yb, vb)
        fb_verdict(x0, y0, x, y, v, xb, yb, vb, dist)
        if i % 3 == 0:
            f.replace_mask(fr[i], x, y, v, mask)
        rows.append((x.copy(), y.copy(), v.copy()))
    f.close()
    b.close()
    want = tuple(np.stack([r[k] for r in rows]) for k in range(3))
    V = want[2]
    assert (V == FB_REJECTED).sum() >= 5 and sum(int((V[j] > 0).sum()) for j in (2, 5, 8, 11)) >= 20
    for j in (2, 5, 8, 11):
        got = V[j] > 0
        assert (mask[want[1][j][got].astype(int), want[0][j][got].astype(int)] != 0).all()
    d = dev(fr, placed_list(), mask=mask, flags=ms.MASK_SELECT)
    rd = ReplaceDesc.from_tc(d.tc.contents, 3)
    assert gpu.klt_hip_set_fb(d.ctx, 1, dist) == 0
    assert gpu.klt_hip_set_frames_replace(d.ctx, C.byref(rd)) == 0
    d.begin()
    rc = d.track_frames(0, T, 4)
    d.check(gpu, d.ctx, rc, "frames")
    assert_rows_equal(d.tables(), want)


def test_selection_bit_with_the_multi_sequence_replacement(gpu, dev):
    """klt_hip_track_frames_multi_replace on scenes 7 and 8 with one selection
    mask for both: per sequence the shim's loop (orc_track, orc_replace_mask)."""
    from kltamd.device import ReplaceDesc
    mask = ms.scene_mask()
    wants = [ms.shim_table(("multi", s), scene(s), placed_list(), track_mask=None, select_mask=mask, every=3)[:3]
             for s in ms.SEEDS]
    plain = [ms.shim_table(("multi_plain", s), scene(s), placed_list(), every=3)[:3] for s in ms.SEEDS]
    for w, p in zip(wants, plain):
        assert sum(int((w[2][j] > 0).sum()) for j in (2, 5, 8, 11)) >= 20
        assert any(not np.array_equal(a, b) for a, b in zip(w, p))  # the mask changes the replacement
    n1 = len(placed_list()[0])
    start = tuple(np.concatenate([a, a]) for a in placed_list())
    stack = np.stack([np.stack(scene(s)) for s in ms.SEEDS])  # [2, T + 1, H, W]
    d = dev(list(stack.reshape(-1, H, W)), start, mask=mask, flags=ms.MASK_SELECT)
    n = d.n
    rd = ReplaceDesc.from_tc(d.tc.contents, 3)
    counts = (C.c_int * 2)(n1, n1)
    fs = W * H
    tx, ty, tv = (d.up(np.full((T, n), 7.0, F32)) for _ in range(3))
    changed = np.zeros(n, np.uint8)
    runs, filled = (C.c_long * 2)(), (C.c_long * 2)()
    rc = gpu.klt_hip_track_frames_multi_replace(d.ctx, C.byref(d.pd), C.byref(d.td), C.byref(rd), 0, d.dfr, W, fs,
                                                (T + 1) * fs, 2, T, 4, counts, *d.list, tx, ty, tv, n, changed.ctypes.data,
                                                runs, filled)
    d.check(gpu, d.ctx, rc, "multi_replace")
    got = tuple(d.get(t, (T, n), np.int32 if k == 2 else F32) for k, t in enumerate((tx, ty, tv)))
    for s in range(2):
        assert_rows_equal(tuple(np.ascontiguousarray(g[:, s * n1:(s + 1) * n1]) for g in got), wants[s])
    assert runs[0] == 4 and runs[1] == 4 and filled[0] + filled[1] >= 40
