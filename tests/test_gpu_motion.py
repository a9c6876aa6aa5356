"""Every tracker path on the rotating scenes of tests/motion_scenes.py.

klt_synth_frame, which every other test of the batched, multi-sequence,
replacing, lazy-gradient, scheduled and sharded trackers draws its frames from,
only ever loses features out of bounds and moves them by (-0.7, -0.3) px.  On
these scenes features move by up to 6 px in both directions of x and y and are
lost in all four ways (KLT_OOB, KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS,
KLT_SMALL_DET), in every chunk of the sequence.

Every comparison is x and y by bit pattern and val exactly, every table row and
the final list, against the CPU oracle -- which tests/test_motion_host.py holds
to the reference's recorded tables -- and, where one is recorded, against the
reference's table itself.  Each case first asserts its floor on the oracle's
table (motion_scenes.check_*), so a case that stops being real fails.

Common shape: 160x120 frames, 13 tracked frames in chunks of 4 (four chunks,
the last one ragged); 320x240x11 for the sharded cases.
"""
from __future__ import annotations


import numpy as np
import pytest

import motion_scenes as ms
from kltabi import OracleTracker
from test_fb import FB_REJECTED
from test_gpu_fb import batch_fb
from test_gpu_fb import want as fb_want
from test_gpu_multi import Dev, empty, frames_of, start_of
from test_gpu_multi_replace import run_batch, the_same
from test_gpu_multi_replace import single as replace_single
from test_gpu_replace import device_run, oracle_loop, run_klt
from test_gpu_track import _seq_via_api
from test_shard import c_sharded_sequence, sharded_sequence

pytestmark = pytest.mark.gpu

T = ms.NFRAMES - 1
SYNTH = 160120  # a klt_synth_frame sequence beside the scenes in the multi-sequence batches

_singles: dict = {}


@pytest.fixture(scope="module")
def rec():
    with np.load(ms.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def assert_rows(got, want, what, final=None):
    """got, want: X, Y, V [rows, n].  Names the first differing (row, feature)
    and the oracle's status there; final: the list that must equal the last row."""
    X, Y, V = (np.asarray(a) for a in got[:3])
    OX, OY, OV = (np.asarray(a) for a in want[:3])
    assert X.shape == OX.shape and V.shape == OV.shape, (what, X.shape, OX.shape)
    bad = (X.view(np.int32) != OX.view(np.int32)) | (Y.view(np.int32) != OY.view(np.int32)) | (V != OV)
    if bad.any():
        j, k = (int(i) for i in np.argwhere(bad)[0])
        before = f"; the row before: ({OX[j - 1, k]!r}, {OY[j - 1, k]!r}, {OV[j - 1, k]})" if j else ""
        raise AssertionError(f"{what}: {int(bad.sum())} cells differ, first at row {j}, feature {k}: got "
                             f"({X[j, k]!r}, {Y[j, k]!r}, {V[j, k]}), want ({OX[j, k]!r}, {OY[j, k]!r}, {OV[j, k]})"
                             + before)
    if final is not None:
        for f, o in zip(final, (OX[-1], OY[-1], OV[-1])):
            assert np.asarray(f).tobytes() == o.tobytes(), f"{what}: the final list is not the last row"


def recorded(rec, name, seed):
    return tuple(rec[f"{name}_{seed}_{k}"] for k in "XYV")


def placed_single(gpu, seed, name="default", chunk=4, calls=None, hook=None):
    """The placed list on one scene through klt_hip_frames_begin + klt_hip_track_frames."""
    d = Dev(gpu, setup=ms.tc_setup(gpu, name))
    if hook:
        d.ok(getattr(gpu, hook[0])(d.ctx, hook[1]), hook[0])
    out = d.single(ms.scene(seed), ms.placed_list(), chunk=chunk, calls=calls)
    kernel, nlevels = d.kernel(), d.pd.nlevels
    d.close()
    return out, kernel, nlevels


# ---------------------------------------------------------------------------
# a. the one-sequence batched call (k_track7, lazy gradients)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("chunk,calls", [(1, None), (4, None), (64, None), (4, [3, 4, 6])])
def test_batched_call(gpu, oracle, rec, seed, chunk, calls):
    want = ms.oracle_placed(oracle, seed)
    ms.check_placed("default", want)
    out, kernel, _ = placed_single(gpu, seed, chunk=chunk, calls=calls)
    assert kernel.startswith(b"kltdev::k_track7")
    assert_rows(out, want, f"scene {seed}, chunk {chunk}, calls {calls}", final=out[3:])
    if (seed, chunk, calls) == (7, 4, None):
        assert_rows(out, recorded(rec, "default", 7), "scene 7 against the reference's table")


# ---------------------------------------------------------------------------
# b. the tuning hooks change no byte
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hook,value", [("klt_hip_set_lazy_grad", 0), ("klt_hip_set_track_merge", 0),
                                        ("klt_hip_set_track_prio", 0), ("klt_hip_set_track_order", 1),
                                        ("klt_hip_set_track_patch", 0), ("klt_hip_set_frames_overlap", 2)])
def test_tuning_hooks_do_not_change_the_bytes(gpu, oracle, hook, value):
    want = ms.oracle_placed(oracle, 8)
    ms.check_placed("default", want)
    if "plain" not in _singles:
        _singles["plain"] = placed_single(gpu, 8)[0]
    out, _, _ = placed_single(gpu, 8, hook=(hook, value))
    for g, p in zip(out, _singles["plain"]):
        assert g.tobytes() == p.tobytes(), hook
    assert_rows(out, want, f"{hook} {value}", final=out[3:])


# ---------------------------------------------------------------------------
# c. the klt.h surface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("sequential", [True, False])
def test_klt_track_features_loop(gpu, oracle, rec, seed, sequential):
    ms.check_placed("default", ms.oracle_placed(oracle, seed))
    out, _, _ = run_klt(gpu, ms.scene(seed), ms.placed_list(), 64, batched=False, sequential=sequential)
    assert_rows(out[6:], recorded(rec, "default", seed), f"KLTTrackFeatures loop, scene {seed}", final=out[:3])


@pytest.mark.parametrize("seed", ms.SCENES)
def test_klt_track_sequence_from_a_selection(gpu, oracle, seed):
    fr = ms.scene(seed)
    OX, OY, OV = OracleTracker(oracle).harness(fr, 100, ms.NFRAMES, first=fr[0])
    start = ms.selected_start(oracle, seed, 100)
    c = ms.status_counts(OV[:, :T].T, start[2])
    assert c["NOT_FOUND"] >= 20 and c["OOB"] >= 6 and c["LARGE_RESIDUE"] >= 12 and c["alive"] >= 7, c
    X, Y, V, last = _seq_via_api(gpu, list(fr), 100)
    assert_rows((X.T, Y.T, V.T), (OX[:, :T].T, OY[:, :T].T, OV[:, :T].T), f"KLTTrackSequence, scene {seed}", final=last)


# ---------------------------------------------------------------------------
# d. other configurations through the batched call
# ---------------------------------------------------------------------------
# step2 and residue3 were not measured in advance; the oracle's first losses on scene 7:
#   step2     OOB 33  LARGE_RESIDUE 105  MAX_ITERATIONS 71  SMALL_DET 7  alive 35
#   residue3  OOB 19  LARGE_RESIDUE 181  MAX_ITERATIONS 5   SMALL_DET 7  alive 39
@pytest.mark.parametrize("name", ["maxit3", "lighting", "win9", "one_level", "step2", "residue3"])
def test_other_configurations(gpu, oracle, name):
    want = ms.oracle_placed(oracle, 7, name)
    ms.check_placed(name, want)
    out, _, nlevels = placed_single(gpu, 7, name)
    assert nlevels == (1 if name == "one_level" else 2)
    assert_rows(out, want, name, final=out[3:])


# ---------------------------------------------------------------------------
# e. the multi-sequence call
# ---------------------------------------------------------------------------
def multi_case(gpu, oracle):
    """Scene 7 placed, scene 8 placed, a klt_synth_frame sequence with 60
    selected, scene 7 with 100 asked of the selection (43 slots stay
    KLT_NOT_FOUND), an empty sequence; each one's separate call, computed once."""
    seqs = [ms.scene(7), ms.scene(8), frames_of(gpu, SYNTH), ms.scene(7), frames_of(gpu, SYNTH)]
    starts = [ms.placed_list(), ms.placed_list(), start_of(gpu, SYNTH, 60), ms.selected_start(oracle, 7, 100), empty()]
    if "multi" not in _singles:
        refs = []
        for fr, st in zip(seqs, starts):
            d = Dev(gpu)
            refs.append(d.single(fr, st))
            d.close()
        _singles["multi"] = refs
    return seqs, starts, _singles["multi"]


@pytest.mark.parametrize("frame_major", [False, True])
def test_multi_sequence_call(gpu, oracle, frame_major):
    seqs, starts, refs = multi_case(gpu, oracle)
    assert (starts[3][2] == ms.NOT_FOUND).sum() >= 20
    for seed in ms.SCENES:
        ms.check_placed("default", ms.oracle_placed(oracle, seed))
    d = Dev(gpu)
    got = d.multi(seqs, starts, frame_major=frame_major)
    assert d.kernel() == b"kltdev::k_track7_multi<2>"
    d.close()
    for s, (g, r) in enumerate(zip(got, refs)):
        assert_rows(g, r, f"sequence {s} against its separate call", final=g[3:])
    for s, seed in enumerate(ms.SCENES):
        assert_rows(got[s], ms.oracle_placed(oracle, seed), f"sequence {s} against the oracle")


@pytest.mark.parametrize("frame_major", [False, True])
def test_more_sequences_than_xcds(gpu, oracle, frame_major):
    """Nine sequences, scenes 7 and 8 in turn, 5..40 of the placed features each
    (features do not interact: the oracle's columns of the whole list)."""
    counts = [5, 9, 14, 18, 23, 27, 32, 36, 40]
    x, y, v = ms.placed_list()
    seeds = [ms.SCENES[s % 2] for s in range(9)]
    picks = [(np.arange(n) * 251 // n + 3 * s) % 251 for s, n in enumerate(counts)]
    wants = [tuple(a[:, idx] for a in ms.oracle_placed(oracle, seed)) for seed, idx in zip(seeds, picks)]
    seen = set()
    for w in wants:
        seen |= {status for _, status in ms.first_losses(w[2])}
    assert seen >= set(ms.LOSSES.values()) and sum((w[2][-1] >= 0).sum() for w in wants) >= 30
    d = Dev(gpu)
    got = d.multi([ms.scene(s) for s in seeds], [(x[i], y[i], v[i]) for i in picks], frame_major=frame_major)
    d.close()
    for s, (g, w) in enumerate(zip(got, wants)):
        assert_rows(g, w, f"sequence {s} of nine", final=g[3:])


# ---------------------------------------------------------------------------
# f. replacement inside the batched call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("chunk", [1, 4])
def test_replacement_in_the_batched_call(gpu, oracle, seed, every, chunk):
    fr = ms.scene(seed)
    start, table, points = oracle_loop(oracle, ("scene", seed), fr, 60, every)
    filled = ms.check_replace(every, points)
    out, (_, counters, _, kernel) = device_run(gpu, fr, start, every, chunk=chunk)
    assert_rows(out, table, f"scene {seed}, every {every}, chunk {chunk}", final=out[3:])
    assert counters == (1, T, sum(1 for _, lost, _ in points if lost), sum(filled))
    assert b"k_track7" in kernel


def test_replacement_against_the_reference_harness(gpu, rec):
    """The reference's own select + track + replace run, 100 features, scene 7."""
    start = tuple(rec[f"sel100_7_{k}"] for k in "xyv")
    want = tuple(rec[f"harness100_7_{k}"][:, :T].T for k in "XYV")
    assert (start[2] == ms.NOT_FOUND).sum() >= 20  # slots the selection left empty ...
    assert (want[2][0] >= 0).sum() > (start[2] >= 0).sum()  # ... some of them filled after the first frame
    out, _ = device_run(gpu, ms.scene(7), start, 1, chunk=4)
    assert_rows(out, want, "the reference's harness with replacement", final=out[3:])


# ---------------------------------------------------------------------------
# g. replacement inside the multi-sequence call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frame_major", [False, True])
def test_replacement_in_the_multi_sequence_call(gpu, oracle, frame_major):
    keys = [("scene", 7), ("scene", 8), SYNTH]
    seqs = [ms.scene(7), ms.scene(8), frames_of(gpu, SYNTH)]
    orc = [oracle_loop(oracle, k, fr, 60, 3) for k, fr in zip(keys, seqs)]
    for o in orc[:2]:
        ms.check_replace(3, o[2])
    starts = [o[0] for o in orc]
    refs = [replace_single(gpu, ("motion", k), fr, st, 3) for k, fr, st in zip(keys, seqs, starts)]
    got, (_, kernel, _) = run_batch(gpu, seqs, starts, 3, frame_major=frame_major)
    assert kernel == b"kltdev::k_track7_multi<2>"
    for s, (g, r, o) in enumerate(zip(got, refs, orc)):
        assert_rows(g[0], o[1], f"sequence {s} against the oracle", final=g[0][3:])
        the_same(g, r)
        assert g[1] == (sum(1 for _, lost, _ in o[2] if lost), sum(p[2] for p in o[2]))


# ---------------------------------------------------------------------------
# h. the forward-backward check, batched
# ---------------------------------------------------------------------------
# max_dist 0.05 on scene 7: the oracle's check rejects 35 features (first losses: OOB 36,
# LARGE_RESIDUE 109, MAX_ITERATIONS 1, SMALL_DET 6; 64 alive at the end)
@pytest.mark.parametrize("chunks,calls", [([3], None), ([2, 7], [3, 10])])
def test_forward_backward_check(gpu, oracle, chunks, calls):
    start = ms.placed_list()
    exp = fb_want(oracle, "motion scene 7", ms.scene(7), len(start[0]), 0.05, start=start)
    OV = exp[2][:, :T].T
    c = ms.status_counts(OV)
    assert exp[4] >= 1 and (OV == FB_REJECTED).any(), "the check rejects nothing"
    assert all(c[s] >= 1 for s in ms.LOSSES) and c["alive"] >= 30, c
    X, Y, V, E = batch_fb(gpu, list(ms.scene(7)), len(start[0]), chunks, 0.05, calls=calls, start=start)
    assert_rows((X, Y, V), (exp[0][:, :T].T, exp[1][:, :T].T, OV), f"forward-backward, chunks {chunks}")
    assert E.view(np.int32).tobytes() == exp[3][:T].view(np.int32).tobytes(), "e differs"


# ---------------------------------------------------------------------------
# i. sharded
# ---------------------------------------------------------------------------
def assert_final(got, table, what):
    x, y, v = got
    bad = (x.view(np.int32) != table[0][-1].view(np.int32)) | (y.view(np.int32) != table[1][-1].view(np.int32)) | (
        v != table[2][-1])
    assert not bad.any(), f"{what}: {int(bad.sum())} features differ, first {int(np.argwhere(bad)[0, 0])}"


@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("world,chunk,margin,band_only", [(3, 4, 0, False), (3, 4, 8, False), (4, 3, 0, True)])
def test_sharded(gpu, oracle, seed, world, chunk, margin, band_only):
    start, table = ms.oracle_shard(oracle, seed)
    ms.check_shard(world, table, start)
    x, y, v, redone = sharded_sequence(gpu, list(ms.shard_scene(seed)), ms.SFEAT, world, chunk, margin,
                                       band_only=band_only)
    assert_final((x, y, v), table, f"scene {seed}, world {world}, margin {margin}")
    if margin == 0:
        assert redone > 0  # no margin: features next to a band edge escape and the chunk is redone


@pytest.mark.parametrize("seed", ms.SCENES)
def test_c_sharded(gpu, oracle, seed):
    start, table = ms.oracle_shard(oracle, seed)
    ms.check_shard(3, table, start)
    x, y, v, redone = c_sharded_sequence(gpu, list(ms.shard_scene(seed)), ms.SFEAT, 3, 4, 0)
    assert_final((x, y, v), table, f"scene {seed}")
    assert redone > 0


@pytest.mark.parametrize("seed", ms.SCENES)
def test_c_sharded_with_replacement(gpu, oracle, seed):
    """KLTReplaceLostFeatures after every frame, as the harness does."""
    fr = ms.shard_scene(seed)
    start, table = ms.oracle_shard(oracle, seed)
    ms.check_shard(3, table, start)
    X, Y, V = OracleTracker(oracle).harness(fr, ms.SFEAT, ms.SFRAMES, first=fr[0], replace=True)
    k = ms.SFRAMES - 2
    assert (V[:, :k + 1] > 0).sum() >= 130  # refilled slots carry their eigenvalue (the oracle: 265 / 270)
    x, y, v, _ = c_sharded_sequence(gpu, list(fr), ms.SFEAT, 3, 1, 8, replace=True)
    assert_final((x, y, v), (X[:, :k + 1].T, Y[:, :k + 1].T, V[:, :k + 1].T), f"scene {seed} with replacement")
