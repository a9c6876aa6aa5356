"""The schedules of a batched call (klt_hip_set_frames_overlap 0..3).

Only the time at which a chunk's pyramids are built differs between one stream,
"automatic", "beside" and "tail", so every case here compares x, y, val and the
table rows byte for byte with the same calls on one stream; one case is held
to the oracle as well.

Common shape: 160x120 frames (level 1 is 40x30), 13 tracked frames in chunks
of 4: four chunks, the last one ragged, every bank reused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import OracleTracker

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, T, CHUNK = 160, 120, 13, 4
ONE, AUTO, BESIDE, TAIL = 0, 1, 2, 3
K_DEFAULT = 3072
FB_REJECTED_DIST = 0.5


@pytest.fixture(scope="module")
def frames(gpu):
    return synth(gpu, 160120, W, H, T + 1)


def _select(gpu, frames, n):
    from kltabi import fl_to_arrays, u8ptr
    tc = gpu.KLTCreateTrackingContext()
    fl = gpu.KLTCreateFeatureList(n)
    gpu.KLTSelectGoodFeatures(tc, u8ptr(np.ascontiguousarray(frames[0])), W, H, fl)
    x, y, v = fl_to_arrays(fl)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    return x, y, v


def run(gpu, frames, start, calls, lazy=1, budget=None, chunk_seen=None):
    """klt_hip_frames_begin on frames[0], then one klt_hip_track_frames call per
    entry of `calls` -- dict(nf=frames, mode=schedule, k=waves left or None,
    chunk=frames per chunk, fb=forward-backward check on) -- from the list
    `start` (x, y, val).  Returns the table [T, n] and the final list."""
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check
    x, y, v = (np.ascontiguousarray(a).copy() for a in start)
    n = len(x)
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_set_lazy_grad(ctx, lazy) == 0
    if budget is not None:
        assert gpu.klt_hip_set_bank_budget(ctx, budget) == 0
    stack = np.ascontiguousarray(np.stack(frames))
    m = max(n, 1)
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    dx, dy, dv = (gpu.klt_hip_malloc(ctx, 4 * m) for _ in range(3))
    tx, ty, tv = (gpu.klt_hip_malloc(ctx, 4 * m * T) for _ in range(3))
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    if n:
        for d, a in ((dx, x), (dy, y), (dv, v)):
            check(gpu, ctx, gpu.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
    j0 = 0
    for call in calls:
        check(gpu, ctx, gpu.klt_hip_set_frames_overlap(ctx, call["mode"]), "schedule")
        if call.get("k") is not None:
            check(gpu, ctx, gpu.klt_hip_set_frames_tail(ctx, call["k"]), "tail")
        if call.get("fb"):
            check(gpu, ctx, gpu.klt_hip_set_fb(ctx, 1, FB_REJECTED_DIST), "fb on")
        off = 4 * n * j0
        check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + (1 + j0) * W * H, W, W * H,
                                                 call["nf"], call.get("chunk", CHUNK), dx, dy, dv, n, tx + off,
                                                 ty + off, tv + off, n), "frames")
        if chunk_seen is not None:
            chunk_seen.append(gpu.klt_hip_frames_chunk(ctx))
        if call.get("fb"):
            check(gpu, ctx, gpu.klt_hip_set_fb(ctx, 0, 0.0), "fb off")
        j0 += call["nf"]
    assert j0 == T
    X, Y, V = np.empty((T, n), F32), np.empty((T, n), F32), np.empty((T, n), np.int32)
    check(gpu, ctx, gpu.klt_hip_sync(ctx), "sync")
    if n:
        for d, a in ((tx, X), (ty, Y), (tv, V), (dx, x), (dy, y), (dv, v)):
            check(gpu, ctx, gpu.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
    for d in (dfr, dx, dy, dv, tx, ty, tv):
        gpu.klt_hip_free(ctx, d)
    gpu.KLTFreeTrackingContext(tc)
    return X, Y, V, x, y, v


def same(a, b):
    for p, q in zip(a, b):
        assert p.shape == q.shape
        assert p.tobytes() == q.tobytes()


_starts, _refs = {}, {}


def start_of(gpu, frames, n):
    if n not in _starts:
        _starts[n] = _select(gpu, frames, n) if n else (np.empty(0, F32), np.empty(0, F32), np.empty(0, np.int32))
    return _starts[n]


def reference(gpu, frames, n, lazy):
    """The whole sequence in one call on one stream, computed once."""
    if (n, lazy) not in _refs:
        _refs[n, lazy] = run(gpu, frames, start_of(gpu, frames, n), [dict(nf=T, mode=ONE)], lazy=lazy)
    return _refs[n, lazy]


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 7, 300])
@pytest.mark.parametrize("mode,k", [(AUTO, None), (BESIDE, None), (TAIL, None), (TAIL, 0), (TAIL, 1), (TAIL, 10 ** 6)])
def test_every_schedule_gives_the_same_bytes(gpu, frames, n, lazy, mode, k):
    """No launch (n = 0), a partial workgroup (1: three of its four waves return
    before tracking; 7: one of the second workgroup's), several workgroups
    (300: most of the list is never found on a frame this small, so many waves
    leave at once).  Tail with its default K, with no wave left, with one, and
    with more than are launched (no wait at all)."""
    got = run(gpu, frames, start_of(gpu, frames, n), [dict(nf=T, mode=mode, k=k)], lazy=lazy)
    same(got, reference(gpu, frames, n, lazy))


def test_tail_vs_oracle(gpu, oracle, frames):
    X, Y, V, *_ = run(gpu, frames, start_of(gpu, frames, 300), [dict(nf=T, mode=TAIL, k=1)])
    OX, OY, OV = OracleTracker(oracle).harness(frames, 300, T + 1, first=frames[0])
    assert (OV[:, T - 1] == 0).sum() > 10  # the case is real: features survive the sequence
    for j in range(T):
        assert np.array_equal(V[j], OV[:, j])
        assert np.array_equal(X[j].view(np.int32), OX[:, j].view(np.int32))
        assert np.array_equal(Y[j].view(np.int32), OY[:, j].view(np.int32))


def test_xcd_ordered_launch_with_padding_blocks(gpu, frames):
    """2049 hand-placed features: past the processing order's threshold, 513
    workgroups in XCD-major order over a grid of 8 x 65, so seven blocks (and
    three waves of the last real one) return before tracking and still count.
    2080 waves: the default K releases the build at once, 1024 half-way."""
    rng = np.random.default_rng(2049)
    n = 2049
    start = (rng.uniform(30, W - 30, n).astype(F32), rng.uniform(30, H - 30, n).astype(F32), np.zeros(n, np.int32))
    ref = run(gpu, frames, start, [dict(nf=T, mode=ONE)])
    assert (ref[2][-1] == 0).sum() > 100
    for k in (0, 1, 1024, K_DEFAULT, 10 ** 6):
        same(run(gpu, frames, start, [dict(nf=T, mode=TAIL, k=k)]), ref)


@pytest.mark.parametrize("modes", [(TAIL, ONE), (ONE, TAIL), (TAIL, BESIDE), (BESIDE, TAIL), (TAIL, TAIL), (AUTO, TAIL)])
def test_mode_changed_between_two_calls(gpu, frames, modes):
    """Two calls on one context (9 + 4 frames in chunks of 2, so both span
    several chunks); the second tail call continues the first one's count."""
    start = start_of(gpu, frames, 300)
    calls = [dict(nf=9, mode=modes[0], k=1, chunk=2), dict(nf=4, mode=modes[1], k=2, chunk=2)]
    same(run(gpu, frames, start, calls), reference(gpu, frames, 300, 1))


@pytest.mark.parametrize("mode", [AUTO, BESIDE, TAIL])
def test_lazy_call_then_forward_backward_call(gpu, frames, mode):
    """The kept image-only frame is made whole between the calls; the forward-
    backward kernels do not count exits, so a tail call with the check on runs
    as "beside" and the count stays where the lazy call left it."""
    start = start_of(gpu, frames, 300)
    plan = lambda m: [dict(nf=8, mode=m, k=1), dict(nf=5, mode=m, k=1, chunk=2, fb=True)]
    ref = run(gpu, frames, start, plan(ONE))
    assert (ref[2][-1] == 0).sum() > 10
    same(run(gpu, frames, start, plan(mode)), ref)


def test_every_feature_lost_in_the_first_chunk(gpu, frames):
    """Features whose level-1 position fails the window bounds test are out of
    bounds after the first frame: every wave of the later launches leaves at
    once, and the builds still follow."""
    n = 300
    start = (np.full(n, 5.0, F32), np.linspace(4.0, 8.0, n).astype(F32), np.zeros(n, np.int32))
    ref = run(gpu, frames, start, [dict(nf=T, mode=ONE)])
    assert (ref[2][CHUNK - 1] < 0).all()
    for k in (0, 1, K_DEFAULT):
        same(run(gpu, frames, start, [dict(nf=T, mode=TAIL, k=k)]), ref)


def test_reduced_bank_budget(gpu, frames):
    """A budget that holds at most two frames per bank: the call runs shorter
    chunks than the four it asked for, so more launches and more waits."""
    seen = []
    got = run(gpu, frames, start_of(gpu, frames, 300), [dict(nf=T, mode=TAIL, k=1)], budget=2_000_000, chunk_seen=seen)
    assert 1 <= seen[0] < CHUNK, seen
    same(got, reference(gpu, frames, 300, 1))


def test_setter_refuses_unknown_schedules(gpu):
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    for bad in (-1, 4):
        assert gpu.klt_hip_set_frames_overlap(ctx, bad) != 0
    assert gpu.klt_hip_set_frames_tail(ctx, -1) != 0
    for ok in (ONE, AUTO, BESIDE, TAIL):
        assert gpu.klt_hip_set_frames_overlap(ctx, ok) == 0
    gpu.KLTFreeTrackingContext(tc)
