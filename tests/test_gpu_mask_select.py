"""The region mask's selection use on the GPU (klt_hip_set_mask with
KLT_HIP_MASK_SELECT) against its CPU statement (tests/native/mask_oracle.c:
orc_select_mask / orc_replace_mask), bit for bit, `changed` marks included:
klt_hip_select (select-all, then replace), klt_hip_select_dev_map and
klt_hip_select_map, on images_provided/img0 (320x240, 150 features) and one
160x120 scene frame."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import mask_scenes as ms
from gpu_helpers import Dev
from kltabi import OracleParams, load_dataset
from motion_scenes import F32, placed_list, scene
from test_mask_host import bits, img0_mask, same

pytestmark = pytest.mark.gpu

N = 150


class SelDev(Dev):
    """gpu_helpers.Dev with a mask in device memory and the selection calls on host lists."""

    def __init__(self, lib, setup=None):
        super().__init__(lib, setup)
        self.bufs = []

    def upload(self, a):
        from kltamd.device import H2D, check
        a = np.ascontiguousarray(a)
        d = self.lib.klt_hip_malloc(self.ctx, max(a.nbytes, 1))
        assert d
        self.bufs.append(d)
        check(self.lib, self.ctx, self.lib.klt_hip_memcpy(self.ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        return d

    def download(self, d, n, dtype):
        from kltamd.device import D2H, check
        a = np.empty(n, dtype)
        check(self.lib, self.ctx, self.lib.klt_hip_memcpy(self.ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return a

    def set_mask(self, mask, flags=ms.MASK_SELECT):
        """mask: [H, pitch] uint8 or None."""
        if mask is None:
            assert self.lib.klt_hip_set_mask(self.ctx, None, 0, 0) == 0
            return None
        d = self.upload(mask)
        assert self.lib.klt_hip_set_mask(self.ctx, d, mask.shape[1], flags) == 0
        return d

    def sd(self):
        from kltamd.device import SelectDesc
        t = self.tc.contents
        return SelectDesc(t.window_width, t.window_height, max(t.borderx, t.window_width // 2),
                          max(t.bordery, t.window_height // 2), t.nSkippedPixels)

    def select(self, img, start, overwrite_all, slot=2):
        """klt_hip_select on a selection image of `img` (as KLTSelectGoodFeatures builds it)."""
        t = self.tc.contents
        h, w = img.shape
        self.build(img, slot=slot, nlevels=1, smooth=t.smoothBeforeSelecting)
        x, y, v = (np.array(a) for a in start)
        ch = np.full(len(x), 9, np.uint8)
        sd = self.sd()
        rc = self.lib.klt_hip_select(self.ctx, slot, C.byref(sd), w, h, t.mindist, t.min_eigenvalue, overwrite_all,
                                     x.ctypes.data, y.ctypes.data, v.ctypes.data, ch.ctypes.data, len(x))
        return rc, (x, y, v), ch

    def select_dev_map(self, img, start, overwrite_all, slot=2):
        t = self.tc.contents
        h, w = img.shape
        self.build(img, slot=slot, nlevels=1, smooth=t.smoothBeforeSelecting)
        emap, nx, ny = self.eigen(slot)
        dmap = self.upload(emap)
        x, y, v = (np.array(a) for a in start)
        ch = np.full(len(x), 9, np.uint8)
        sd = self.sd()
        rc = self.lib.klt_hip_select_dev_map(self.ctx, dmap, nx, ny, C.byref(sd), w, h, t.mindist, t.min_eigenvalue,
                                             overwrite_all, x.ctypes.data, y.ctypes.data, v.ctypes.data, ch.ctypes.data,
                                             len(x))
        return rc, (x, y, v), ch

    def error(self):
        m = self.lib.klt_hip_last_error(self.ctx)
        return m.decode() if m else ""

    def close(self):
        if self.tc:
            self.lib.klt_hip_sync(self.ctx)
            self.lib.klt_hip_set_mask(self.ctx, None, 0, 0)
            for d in self.bufs:
                self.lib.klt_hip_free(self.ctx, d)
        super().close()


@pytest.fixture
def dev(gpu):
    made = []

    def make(setup=None):
        made.append(SelDev(gpu, setup))
        return made[-1]
    yield make
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def img0():
    return load_dataset(n=1)[0]


def zeros(n=N):
    return np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, np.int32)


def shim_params(skip=0):
    p = OracleParams()
    ms.load_shim().orc_default_params(C.byref(p))
    p.nSkippedPixels = skip
    return p


def lose_a_third(lst):
    x, y, v = (a.copy() for a in lst)
    v[::3] = -3
    return x, y, v


def want_select(img, mask, skip=0):
    """The shim's selection and, from it with a third of the list lost, its replacement (no kept pyramid)."""
    s = ms.Shim(shim_params(skip), sequential=0)
    sel = s.select_mask(img, N, mask)
    rep = lose_a_third(sel)
    s.replace_mask(img, *rep, mask)
    s.close()
    return sel, rep


def check_mask_bites(img, mask, sel, plain):
    """At least a quarter of the unmasked selection lies on masked pixels; no selected feature does."""
    ok = plain[2] > 0
    on = (mask[plain[1][ok].astype(int), plain[0][ok].astype(int)] == 0).sum()
    assert on * 4 >= ok.sum(), (on, ok.sum())
    got = sel[2] > 0
    assert got.sum() >= N // 2 and (mask[sel[1][got].astype(int), sel[0][got].astype(int)] != 0).all()


@pytest.mark.parametrize("call", ["select", "select_dev_map"])
@pytest.mark.parametrize("skip", [0, 1])
def test_select_and_replace_vs_shim(gpu, dev, img0, call, skip):
    mask, plain = img0_mask(img0)
    h, w = img0.shape
    sel, rep = want_select(img0, mask, skip)
    if skip == 0:
        check_mask_bites(img0, mask, sel, plain)
    else:  # the grid-to-pixel map: only even offsets from the border are grid points
        got = sel[2] > 0
        assert got.sum() >= N // 2 and (mask[sel[1][got].astype(int), sel[0][got].astype(int)] != 0).all()
        assert not same(sel, want_select(img0, mask, 0)[0])

    def setup(t):
        t.nSkippedPixels = skip
    d = dev(setup)
    d.set_mask(mask)
    fn = getattr(d, call)
    rc, got, ch = fn(img0, zeros(), 1)
    assert rc == 0, d.error()
    assert same(got, sel) and (ch == 1).all()
    # replacement after losing a third of the list
    lost = lose_a_third(sel)
    rc, got, ch = fn(img0, lost, 0)
    assert rc == 0, d.error()
    assert same(got, rep)
    assert np.array_equal(ch, (lost[2] < 0).astype(np.uint8))
    live = rep[2] >= 0
    assert (mask[rep[1][live].astype(int), rep[0][live].astype(int)] != 0)[lost[2][live] < 0].all()
    assert ((rep[2] > 0) & (lost[2] < 0)).sum() >= 10  # slots were refilled


@pytest.mark.parametrize("call", ["select", "select_dev_map"])
def test_all_allowed_null_clear_and_reset_give_todays_bytes(gpu, dev, img0, call):
    mask, plain = img0_mask(img0)
    h, w = img0.shape
    d = dev()
    fn = getattr(d, call)
    rc, none, ch0 = fn(img0, zeros(), 1)
    assert rc == 0 and same(none, plain)
    lost = lose_a_third(plain)
    rc, none_rep, chr0 = fn(img0, lost, 0)
    assert rc == 0
    # all allowed
    d.set_mask(np.ones((h, w), np.uint8))
    rc, got, ch = fn(img0, zeros(), 1)
    assert rc == 0 and same(got, none) and np.array_equal(ch, ch0)
    rc, got, ch = fn(img0, lost, 0)
    assert rc == 0 and same(got, none_rep) and np.array_equal(ch, chr0)
    # the mask bites, then is cleared
    d.set_mask(mask)
    rc, got, ch = fn(img0, zeros(), 1)
    assert rc == 0 and not same(got, none)
    d.set_mask(None)
    rc, got, ch = fn(img0, zeros(), 1)
    assert rc == 0 and same(got, none)
    # ... and klt_hip_ctx_reset clears it
    dm = d.set_mask(mask)
    p, pitch, flags = C.c_void_p(), C.c_long(), C.c_int()
    assert gpu.klt_hip_get_mask(d.ctx, C.byref(p), C.byref(pitch), C.byref(flags)) == 0
    assert (p.value, pitch.value, flags.value) == (dm, w, ms.MASK_SELECT)
    assert gpu.klt_hip_ctx_reset(d.ctx) == 0
    assert gpu.klt_hip_get_mask(d.ctx, C.byref(p), C.byref(pitch), C.byref(flags)) == 0
    assert (p.value, pitch.value, flags.value) == (None, 0, 0)
    rc, got, ch = fn(img0, zeros(), 1)
    assert rc == 0 and same(got, none)


def test_all_masked_selects_nothing(gpu, dev, img0):
    h, w = img0.shape
    d = dev()
    d.set_mask(np.zeros((h, w), np.uint8))
    rc, (x, y, v), ch = d.select(img0, zeros(), 1)
    assert rc == 0 and (v == -1).all() and (x == -1).all() and (y == -1).all() and (ch == 1).all()


@pytest.mark.parametrize("pad", [0, 1])
def test_pitch_wider_than_the_image(gpu, dev, img0, pad):
    """The padding past column ncols holds the opposite of most of the mask (pad
    0) or of its zero regions (pad 1): it is never read as a pixel."""
    mask, plain = img0_mask(img0)
    h, w = img0.shape
    wide = np.full((h, w + 37), pad, np.uint8)
    wide[:, :w] = mask
    sel, rep = want_select(img0, mask)
    d = dev()
    d.set_mask(wide)
    rc, got, ch = d.select(img0, zeros(), 1)
    assert rc == 0 and same(got, sel)
    rc, got, ch = d.select(img0, lose_a_third(sel), 0)
    assert rc == 0 and same(got, rep)


def test_bad_flags_and_short_pitch(gpu, dev, img0):
    mask, plain = img0_mask(img0)
    h, w = img0.shape
    d = dev()
    dm = d.set_mask(mask)
    # flags outside the two bits: -1, the setting unchanged
    assert gpu.klt_hip_set_mask(d.ctx, dm, w, 4) == -1 and "set_mask" in d.error()
    assert gpu.klt_hip_set_mask(d.ctx, dm, w, ms.MASK_SELECT | 8) == -1
    p, pitch, flags = C.c_void_p(), C.c_long(), C.c_int()
    assert gpu.klt_hip_get_mask(d.ctx, C.byref(p), C.byref(pitch), C.byref(flags)) == 0
    assert (p.value, pitch.value, flags.value) == (dm, w, ms.MASK_SELECT)
    # a pitch below the image's width: refused by the call that learns the width, lists untouched
    assert gpu.klt_hip_set_mask(d.ctx, dm, w - 1, ms.MASK_SELECT) == 0
    start = lose_a_third(plain)
    for call in (d.select, d.select_dev_map):
        rc, got, ch = call(img0, start, 0)
        assert rc == -1 and "klt_hip_set_mask" in d.error(), d.error()
        assert same(got, start) and (ch == 9).all()


def test_select_map_on_a_scene_frame(gpu, dev):
    """klt_hip_select_map (the sharded replacement's selection) reads the kept
    pyramid's level 0: frame 1 of the 160x120 scene after one tracked frame,
    against orc_track + orc_replace_mask in sequential mode."""
    from kltamd.device import PyrDesc, check
    fr = scene(7)
    h, w = fr[1].shape

    def shim(m):
        """One tracked frame, seven of eight slots then lost, orc_replace_mask on the kept pyramid."""
        s = ms.Shim()
        x, y, v = (a.copy() for a in placed_list())
        s.track_mask(fr[0], fr[1], x, y, v, None)
        drop = np.arange(len(x)) % 8 != 0
        x[drop], y[drop], v[drop] = -1.0, -1.0, -3
        lost = (x.copy(), y.copy(), v.copy())
        s.replace_mask(fr[1], x, y, v, m)
        s.close()
        return lost, (x, y, v)

    # the mask: squares around every second feature the unmasked replacement places
    lost, (px, py, pv) = shim(None)
    pf = np.nonzero((lost[2] < 0) & (pv > 0))[0]
    mask = np.ones((h, w), np.uint8)
    for k in pf[::2]:
        mask[int(py[k]) - 4:int(py[k]) + 5, int(px[k]) - 4:int(px[k]) + 5] = 0
    assert len(pf) >= 20 and (mask[py[pf].astype(int), px[pf].astype(int)] == 0).sum() * 4 >= len(pf)
    lost, (x, y, v) = shim(mask)
    filled = (lost[2] < 0) & (v > 0)
    assert filled.sum() >= 20 and (mask[y[filled].astype(int), x[filled].astype(int)] != 0).all()

    d = dev()
    d.tc.contents.sequentialMode = 1
    g, ctx = gpu, d.ctx
    pd = d.desc(w, h)
    dfr = d.upload(fr[1])
    check(g, ctx, g.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    sd = d.sd()
    nx, ny, j0, j1 = (C.c_int() for _ in range(4))
    assert g.klt_hip_min_eigen_rows(ctx, C.byref(sd), 0, h, None, C.byref(nx), C.byref(ny), C.byref(j0), C.byref(j1)) == 0
    dmap = d.upload(np.zeros(nx.value * ny.value, np.int32))
    assert g.klt_hip_min_eigen_rows(ctx, C.byref(sd), 0, h, dmap, C.byref(nx), C.byref(ny), C.byref(j0), C.byref(j1)) == 0
    t = d.tc.contents
    n = len(x)

    def run(mask_arr, pitch=None):
        d.set_mask(mask_arr)
        if pitch is not None:
            assert g.klt_hip_set_mask(ctx, d.bufs[-1], pitch, ms.MASK_SELECT) == 0
        lists = [d.upload(a) for a in lost]
        rc = g.klt_hip_select_map(ctx, w, h, C.byref(sd), t.mindist, t.min_eigenvalue, dmap, *lists, n)
        return rc, tuple(d.download(p, n, np.int32 if k == 2 else F32) for k, p in enumerate(lists))

    rc, got = run(mask)
    assert rc == 0, d.error()
    assert same(got, (x, y, v))
    rc, got = run(None)
    assert rc == 0 and same(got, (px, py, pv))
    rc, got = run(mask, pitch=w - 1)
    assert rc == -1 and "klt_hip_set_mask" in d.error() and same(got, lost)
