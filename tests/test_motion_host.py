"""The rotating scenes of tests/motion_scenes.py on the CPU: the generator gives
the recorded frames, the oracle gives the reference's recorded tables bit for
bit (tests/golden/motion_160x120.npz, written by tests/golden/make_motion.py
from the reference build), and every floor that tests/test_gpu_motion.py relies
on holds on the oracle's tables."""
from __future__ import annotations

import hashlib
import json

import numpy as np
import pytest

import motion_scenes as ms
from kltabi import GOLDEN, OracleTracker
from test_gpu_replace import oracle_loop


@pytest.fixture(scope="module")
def rec():
    with np.load(ms.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_same_table(got, want, what):
    for g, w, name in zip(got, want, "xyv"):
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(bits(g) != bits(w)) if name != "v" else np.argwhere(g != w)
        assert not len(bad), f"{what}: {name} differs at {len(bad)} cells, first (row, feature) {bad[0].tolist()}"


def test_fixture_is_the_recorded_one():
    man = json.loads((GOLDEN / "manifest.json").read_text())
    assert hashlib.sha256(ms.FIXTURE.read_bytes()).hexdigest() == man[ms.FIXTURE.name]


@pytest.mark.parametrize("seed", ms.SCENES)
def test_generator_reproduces_the_recorded_frames(rec, seed):
    fr = ms.scene(seed)
    assert len(fr) == ms.NFRAMES and fr[0].shape == (ms.H, ms.W) and fr[0].dtype == np.uint8
    assert hashlib.sha256(np.stack(fr).tobytes()).hexdigest() == rec[f"sha_{seed}"].item()
    big = ms.shard_scene(seed)
    assert len(big) == ms.SFRAMES and big[0].shape == (ms.SH, ms.SW)
    assert hashlib.sha256(np.stack(big).tobytes()).hexdigest() == rec[f"sha_shard_{seed}"].item()
    stack = np.stack(fr)
    assert (stack == 0).any() and (stack == 255).any()  # the extremes klt_synth_frame never reaches


def test_placed_list(rec):
    x, y, v = ms.placed_list()
    assert len(x) == 251 and not v.any()
    assert (x[221:] == np.rint(x[221:])).all() and (y[221:] == np.rint(y[221:])).all()  # exact integers
    assert_same_table((x, y, v), (rec["placed_x"], rec["placed_y"], rec["placed_v"]), "placed list")


@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("name", ms.RECORDED)
def test_oracle_equals_the_reference_and_holds_the_floors(oracle, rec, name, seed):
    table = ms.oracle_placed(oracle, seed, name)
    ms.check_placed(name, table)
    assert_same_table(table, tuple(rec[f"{name}_{seed}_{k}"] for k in "XYV"), f"{name}, scene {seed}")


@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("name", ["step2", "residue3"])
def test_unrecorded_configurations_hold_their_floors(oracle, name, seed):
    # the oracle on scenes 7 / 8 (first loss per feature):
    #   step2     OOB 33/31  LARGE_RESIDUE 105/103  MAX_ITERATIONS 71/61  SMALL_DET 7/7  alive 35/49
    #   residue3  OOB 19/14  LARGE_RESIDUE 181/192  MAX_ITERATIONS 5/4    SMALL_DET 7/6  alive 39/35
    ms.check_placed(name, ms.oracle_placed(oracle, seed, name))


@pytest.mark.parametrize("seed", ms.SCENES)
def test_selected_harness_with_replacement(oracle, rec, seed):
    fr = ms.scene(seed)
    start = ms.oracle_select(oracle, fr[0], 100)
    assert_same_table(start, tuple(rec[f"sel100_{seed}_{k}"] for k in "xyv"), f"selection, scene {seed}")
    assert (start[2] == ms.NOT_FOUND).sum() >= 20  # slots the selection leaves empty (the oracle: 43)
    got = OracleTracker(oracle).harness(fr, 100, ms.NFRAMES, first=fr[0], replace=True)
    want = tuple(rec[f"harness100_{seed}_{k}"] for k in "XYV")
    T = ms.NFRAMES - 1  # the last column is never written
    assert_same_table(tuple(g[:, :T].T for g in got), tuple(w[:, :T].T for w in want), f"harness, scene {seed}")
    # the same run without replacement loses features in three ways (the oracle: OOB 14/13,
    # LARGE_RESIDUE 27/25, MAX_ITERATIONS 1/1)
    c = ms.status_counts(ms.oracle_table(oracle, ("sel100", seed), fr, start)[2], start[2])
    assert c["OOB"] >= 6 and c["LARGE_RESIDUE"] >= 12 and c["alive"] >= 7, c


@pytest.mark.parametrize("seed", ms.SCENES)
@pytest.mark.parametrize("every", [1, 3])
def test_replacement_floors(oracle, seed, every):
    _, _, points = oracle_loop(oracle, ("scene", seed), ms.scene(seed), 60, every)
    ms.check_replace(every, points)


@pytest.mark.parametrize("seed", ms.SCENES)
def test_shard_floors(oracle, seed):
    start, table = ms.oracle_shard(oracle, seed)
    c = ms.status_counts(table[2], start[2])
    assert c["OOB"] >= 23 and c["LARGE_RESIDUE"] >= 17 and c["alive"] >= 100, c
    for world in (3, 4):
        ms.check_shard(world, table, start)
