"""One context's bank ring handed from one kind of batched call to the next.

Every batched call runs on the same three banks and the same kept pyramid, so
what one call leaves there -- the layout of each bank, its valid rows, the bank
whose turn is next, a bank built ahead, where the kept pyramid lies -- is what
the next call starts from.  One context makes the calls below one after the
other; each call is also made on a fresh context, started from the same lists
and the same kept frame, and the final x, y, val and every table row must be
the same bytes.

160x120 frames of the synthetic scene 160120, 64 slots, 7 tracked frames in
chunks of 3 (three chunks, the last one ragged, every bank used), under the
automatic schedule:

  1  plain, klt_hip_set_track_impl(1): the generic tracker, banks in planes
  2  klt_hip_track_frames_multi, two sequences (the scene, and the scene one
     frame on): banks laid out again for 2 x 3 pyramids, no kept pyramid after
  3  klt_hip_frames_begin and a plain call: lazy gradients, level 0 of the
     banks the img plane alone, the tail schedule
  4  two band calls of 3 frames (own -inf..inf, rows 0..H): the first builds
     the second's bank ahead, the second builds one that nobody takes.  The
     level-0 launches of each call are counted (klt_hip_set_timing): the second
     call on the one context runs one, its build-ahead, where a fresh context
     runs two
  5  plain: starts from a band bank, overwrites the stale build-ahead
  6  plain with klt_hip_set_frames_replace every 2 frames

Each call starts from a selection on its kept frame (4b from 4a's list), so
features are alive in every one.  Slots tracked at the end of each call, of 64,
counted with the CPU oracle before any GPU run and asserted below on the fresh
contexts: 1: 52, 2: 52 and 51, 3: 52, 4a: 54, 4b: 52, 5: 54, 6: 58.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import fl_to_arrays, u8ptr
from test_gpu_multi import Dev
from test_gpu_replace import same

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, N, T, CHUNK = 160, 120, 64, 7, 3
AUTO = 1
GENERIC = b"kltdev::k_track_frames_g"
MULTI = b"kltdev::k_track7_multi<2>"
LAZY = b"kltdev::k_track7<false, true, 2, false, true>"
BAND = b"kltdev::k_track7<true, true, 2, false>"


def _select(gpu, img):
    tc = gpu.KLTCreateTrackingContext()
    fl = gpu.KLTCreateFeatureList(N)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(img)), W, H, fl)
    out = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    return out


class Ctx(Dev):
    """The calls of this file on one device context; every call returns its
    outputs as host arrays and the tracker kernel's name."""

    def __init__(self, gpu, frames):
        super().__init__(gpu)
        self.ok(gpu.klt_hip_set_frames_overlap(self.ctx, AUTO), "schedule")
        self.dfr = self.up(np.stack(frames))
        self.esc = self.up(np.zeros(1, np.int32))

    def frame(self, k):
        return self.dfr + k * W * H

    def begin(self, k):
        self.ok(self.gpu.klt_hip_frames_begin(self.ctx, C.byref(self.pd), self.frame(k), W), "begin")

    def lists(self, start):
        """x | y | val in one device block, as the replacement's single transfer takes them"""
        n = len(start[0])
        d = self.up(np.concatenate([np.ascontiguousarray(a).view(np.uint32) for a in start]))
        return d, d + 4 * n, d + 8 * n, n

    def out(self, dl, n, tabs=None, rows=T):
        r = tuple(self.down(dl + 4 * n * k, n, t) for k, t in enumerate((F32, F32, np.int32)))
        if tabs:
            r += tuple(self.down(d, (rows, n), t) for d, t in zip(tabs, (F32, F32, np.int32)))
        return r, self.kernel()

    def plain(self, k, start, impl=0, every=0):
        """T frames after the kept frame k, with tables"""
        from kltamd.device import ReplaceDesc
        g = self.gpu
        dx, dy, dv, n = self.lists(start)
        tabs = [self.up(np.zeros(T * n, F32)) for _ in range(3)]
        self.ok(g.klt_hip_set_track_impl(self.ctx, impl), "impl")
        if every:
            rd = ReplaceDesc.from_tc(self.tc.contents, every)
            self.ok(g.klt_hip_set_frames_replace(self.ctx, C.byref(rd)), "replace on")
        self.ok(g.klt_hip_track_frames(self.ctx, C.byref(self.pd), C.byref(self.td), self.frame(k + 1), W, W * H, T, CHUNK,
                                       dx, dy, dv, n, *tabs, n), "frames")
        res = self.out(dx, n, tabs)
        self.ok(g.klt_hip_set_frames_replace(self.ctx, None), "replace off")
        self.ok(g.klt_hip_set_track_impl(self.ctx, 0), "impl")
        return res

    def multi(self, starts):
        """sequence s: the scene from frame s on, its own start image and T frames"""
        S = len(starts)
        x, y, v = (np.concatenate([s[k] for s in starts]) for k in range(3))
        dx, dy, dv, n = self.lists((x, y, v))
        tabs = [self.up(np.zeros(T * n, F32)) for _ in range(3)]
        n_seq = (C.c_int * S)(*[len(s[0]) for s in starts])
        self.ok(self.gpu.klt_hip_track_frames_multi(self.ctx, C.byref(self.pd), C.byref(self.td), self.dfr, W, W * H, W * H, S,
                                                    T, CHUNK, n_seq, dx, dy, dv, *tabs, n), "multi")
        return self.out(dx, n, tabs)

    def band(self, k, start, nf, next_n):
        """nf frames after the kept frame k; the next_n frames after those are the next chunk's"""
        from kltamd.device import Timing
        dx, dy, dv, n = self.lists(start)
        nxt = self.frame(k + 1 + nf) if next_n else None
        self.ok(self.gpu.klt_hip_set_timing(self.ctx, 1), "timing on")
        self.ok(self.gpu.klt_hip_track_frames_band(self.ctx, C.byref(self.pd), C.byref(self.td), self.frame(k + 1), W, W * H,
                                                   nf, dx, dy, dv, n, -np.inf, np.inf, 0, H, self.esc, nxt, next_n), "band")
        tm = Timing()
        self.ok(self.gpu.klt_hip_get_timing(self.ctx, C.byref(tm)), "timing")
        self.ok(self.gpu.klt_hip_set_timing(self.ctx, 0), "timing off")
        self.l0_launches = tm.n_pyr_l0  # this call's own pyramids (unless taken as built ahead) + its build-ahead
        res = self.out(dx, n)
        assert self.down(self.esc, 1, np.int32)[0] == 0  # no window met a missing row
        return res


def tracked(v):
    return int((v >= 0).sum())


def test_the_ring_passes_from_call_to_call(gpu):
    frames = synth(gpu, 160120, W, H, 4 * T + 1)
    sel = {k: _select(gpu, frames[k]) for k in (0, 1, T, 2 * T - 1, 3 * T - 1)}
    one = Ctx(gpu, frames)

    def fresh(call, k=None):
        """`call` on a context of its own, started from the kept frame k"""
        d = Ctx(gpu, frames)
        if k is not None:
            d.begin(k)
        res = call(d)
        d.close()
        return res + (getattr(d, "l0_launches", None),)

    def step(call, k, kernel, least, begin=False):
        """the call on the one context, which stands at frame k, and on a fresh one"""
        if begin:
            one.begin(k)
        got, name = call(one)
        want, name_fresh, l0_fresh = fresh(call, k)
        assert name == name_fresh and name.startswith(kernel), (name, name_fresh)
        for lo, hi, count in least:
            assert tracked(want[2][lo:hi]) >= count, (tracked(want[2][lo:hi]), count)  # the equality below is about live features
        same(got, want)
        return want, l0_fresh

    half = [(0, N, N // 2)]
    # 1: the generic tracker's banks, in planes
    step(lambda d: d.plain(0, sel[0], impl=1), 0, GENERIC, half, begin=True)
    # 2: the banks laid out again for two sequences' pyramids; no kept pyramid afterwards
    n0 = len(sel[0][0])
    step(lambda d: d.multi([sel[0], sel[1]]), None, MULTI, [(0, n0, N // 2), (n0, 2 * N, N // 2)])
    assert gpu.klt_hip_frames_end_slot(one.ctx, 0) == -1 and b"no current pyramid" in one.error()
    # 3: laid out again for one sequence; lazy gradients, image-only level 0
    step(lambda d: d.plain(0, sel[0]), 0, LAZY, half, begin=True)
    # 4: the band calls start from the image-only frame made whole; the second takes the bank built ahead
    a, l0 = step(lambda d: d.band(T, sel[T], 3, 3), T, BAND, half)
    assert (one.l0_launches, l0) == (2, 2)  # its own chunk and the next one's
    _, l0 = step(lambda d: d.band(T + 3, a[:3], 3, 3), T + 3, BAND, half)
    assert (one.l0_launches, l0) == (1, 2)  # the one context took the bank built ahead; a fresh one builds
    # 5: starts from the band call's bank and overwrites the one built ahead for nobody
    step(lambda d: d.plain(2 * T - 1, sel[2 * T - 1]), 2 * T - 1, LAZY, half)
    # 6: the tracker launches cut every 2 frames, lost features replaced in between
    step(lambda d: d.plain(3 * T - 1, sel[3 * T - 1], every=2), 3 * T - 1, LAZY, half)
    one.close()
