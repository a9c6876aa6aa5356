"""The first frame of a lazy-gradient launch and the frames behind it.

k_track7's lazy-gradient instances take image 1 of a launch's first frame from
the kept pyramid -- whole (klt_hip_frames_begin's slot, interleaved records) or
an image-only bank frame left by the lazy call before -- and image 1 of every
later frame from the bank frame just tracked: the level bases are carried from
frame to frame.  The cases here pin what that hand-over can break and the
other files do not: launches of one, two and three frames from both kinds of
kept pyramid, and the deferred residue across a launch's first frame on scenes
that lose features in all four ways.

Every comparison is bit for bit (x and y by pattern, val exactly, every table
row) with the same frames tracked with klt_hip_set_lazy_grad(ctx, 0) -- full
level-0 records, the kernels that carry nothing -- and with the CPU oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

import motion_scenes as ms
from conftest import synth
from kltabi import OracleTracker
from test_gpu_multi import Dev
from test_gpu_track import assert_table_equal, batch_sequence

pytestmark = pytest.mark.gpu

NFEAT = 300
LAZY = b"kltdev::k_track7<false, true, 2, false, true>"
FULL = b"kltdev::k_track7<false, true, 2, false>"


@pytest.fixture(scope="module")
def seq(gpu, oracle):
    """Six 640x480 frames and the oracle's table on them (column j: after frame j + 1)."""
    frames = synth(gpu, 5150, 640, 480, 6)
    want = OracleTracker(oracle).harness(frames, NFEAT, 6, first=frames[0])
    for a in want:
        a.setflags(write=False)
    return frames, want


def run(gpu, frames, on, chunks, calls):
    names = []

    def hook(ctx, done=False):
        if done:
            names.append(gpu.klt_hip_track_kernel(ctx))
        else:
            assert gpu.klt_hip_set_lazy_grad(ctx, on) == 0
    out = batch_sequence(gpu, frames, NFEAT, chunks, calls=calls, ctx_hook=hook)
    assert names == [LAZY if on else FULL], names
    return out


def same_rows(a, b, what):
    for g, w, k in zip(a, b, "xyv"):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("kept", ["whole", "image_only"])
@pytest.mark.parametrize("length", [1, 2, 3])
def test_launch_lengths(gpu, seq, kept, length):
    """A launch of `length` frames: its first frame alone, followed by one
    carried frame, by two.  whole: straight after klt_hip_frames_begin.
    image_only: after a lazy call of two frames (one launch), whose last bank
    frame is the kept pyramid."""
    frames, want = seq
    head = 0 if kept == "whole" else 2
    T = head + length
    calls, chunks = ([length], [64]) if not head else ([head, length], [64, 64])
    on = run(gpu, frames[:T + 1], 1, chunks, calls)
    off = run(gpu, frames[:T + 1], 0, chunks, calls)
    same_rows(on, off, f"{kept}, {length} frame(s), lazy on against off")
    assert_table_equal(*on, *(a[:, :T] for a in want))
    assert (on[2][-1] == 0).sum() > NFEAT // 2  # the case is real: most features are still tracked


_scene_runs: dict = {}


def scene_run(gpu, seed, on, chunk):
    if (seed, on, chunk) not in _scene_runs:
        d = Dev(gpu, setup=ms.tc_setup(gpu, "default"))
        d.ok(gpu.klt_hip_set_lazy_grad(d.ctx, on), "set_lazy_grad")
        out = d.single(ms.scene(seed), ms.placed_list(), chunk=chunk)
        assert d.kernel() == (LAZY if on else FULL), d.kernel()
        d.close()
        _scene_runs[seed, on, chunk] = out
    return _scene_runs[seed, on, chunk]


@pytest.mark.parametrize("chunk", [1, 2, 3])
@pytest.mark.parametrize("seed", ms.SCENES)
def test_deferred_residue_across_the_first_frame(gpu, oracle, seed, chunk):
    """13 frames of a rotating scene in launches of `chunk` frames.  The verdict
    on a launch's first frame arrives with the first carried frame's first pass
    (chunk 2 and 3), the verdict on a launch's last frame is taken in place
    (every chunk; with chunk 1 that is every frame), and features are lost
    with each of the four statuses on the way."""
    want = ms.oracle_placed(oracle, seed)
    ms.check_placed("default", want)
    on = scene_run(gpu, seed, 1, chunk)
    off = scene_run(gpu, seed, 0, 4)
    same_rows(on, off, f"scene {seed}, chunk {chunk}, lazy on against off")
    V = on[2]
    for name, code in ms.LOSSES.items():
        assert (V == code).any(), f"scene {seed}: no feature lost with {name}"
    for g, w, k in zip(on[:3], want[:3], "xyv"):
        w = np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.view(np.int32), w.view(np.int32)), \
            f"scene {seed}, chunk {chunk}: {k} differs from the oracle"
