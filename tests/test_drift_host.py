"""The CPU statement of the drift check (tests/native/drift_oracle.c) held to
the oracle and to its own rules, and the conditions on its tables that a GPU
comparison rests on (drift_scenes.assert_scene_conditions, to be asserted again
before any such comparison).

Measured on motion_scenes.scene (160x120, placed_list()'s 251 features, 13
tracked frames) with max_residue 10: drift_scenes.MEASURED, per configuration,
seed and max_age the features lost to the check, those alive after the last
frame and those lost to the border / a large residue / the iteration limit / a
small determinant while holding a template.  drift_scenes.FLOORS are about half.
"""
from __future__ import annotations

import numpy as np
import pytest

import drift_scenes as ds
from motion_scenes import F32, oracle_placed, placed_list, scene


def bits(a):
    return np.asarray(a).view(np.int32)


def same(a, b):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("seed", ds.SEEDS)
@pytest.mark.parametrize("max_residue", [float("inf"), 1e9], ids=["inf", "1e9"])
def test_unreachable_threshold_is_the_oracle(oracle, seed, max_residue):
    t = ds.placed_table(seed, 0, max_residue=max_residue)
    want = oracle_placed(oracle, seed)
    assert same(t[:3], want)
    assert (t[2][-1] == 0).sum() == ds.ALIVE_OFF[seed]
    assert not (t[2] == ds.DRIFTED).any()
    # the age counts the frames survived: 1 after the frame that stored the template
    V, AGE = t[2], t[4]
    run = np.zeros(V.shape[1], np.int32)
    for j in range(ds.T):
        run = np.where(V[j] == 0, run + 1, 0)
        assert np.array_equal(AGE[j], run), j


@pytest.mark.parametrize("key", sorted(ds.MEASURED), ids=lambda k: "%s-%d-age%d" % k)
def test_scene_conditions(key):
    name, seed, max_age = key
    c = ds.assert_scene_conditions(seed, max_age, name)
    assert c == ds.MEASURED[key]


@pytest.mark.parametrize("seed", ds.SEEDS)
@pytest.mark.parametrize("max_age", ds.AGES)
def test_rules_on_the_table(seed, max_age):
    X, Y, V, E, AGE, TM, B, _ = ds.placed_table(seed, max_age)
    start_v = placed_list()[2]
    prev = np.concatenate([start_v[None], V[:-1]])
    tracked = V == 0
    # rule 1: a slot entering with val != 0 has no template at the frame's start as far as the frame goes:
    # after it the age is 0, or 1 if it was tracked (none re-enters here without a replacement)
    assert (AGE[(prev < 0)] == 0).all()
    # rules 2-4: age after the frame
    tested = E != -1.0
    assert np.array_equal(tested, (prev == 0) & (B > 0) & (tracked | (V == ds.DRIFTED)))
    assert (AGE[~tracked] == 0).all()
    assert (AGE[tracked & (B == 0)] == 1).all()          # stored, no test
    nxt = B + 1
    if max_age:
        nxt = np.where(nxt > max_age, 0, nxt)
        assert B.max() <= max_age and AGE.max() <= max_age
        # a dropped template is stored again on the next tracked frame
        drop = np.argwhere(tracked & (B == max_age))
        assert len(drop) >= 20
        for j, k in drop:
            assert AGE[j, k] == 0
            if j + 1 < ds.T and V[j + 1, k] == 0:
                assert B[j + 1, k] == 0 and AGE[j + 1, k] == 1 and E[j + 1, k] == -1.0
                assert not np.array_equal(bits(TM[j + 1, k]), bits(TM[j, k]))
    assert np.array_equal(AGE[tracked & (B > 0)], nxt[tracked & (B > 0)])
    # rule 4: the verdict is the comparison
    assert (E[(V == ds.DRIFTED) & (prev == 0)] > ds.MAX_RESIDUE).all() and (E[tested & tracked] <= ds.MAX_RESIDUE).all()
    assert (X[V == ds.DRIFTED] == -1).all() and (Y[V == ds.DRIFTED] == -1).all()
    for j, k in np.argwhere((V == ds.DRIFTED) & (prev == 0)):
        assert (V[j:, k] == ds.DRIFTED).all()            # lost from that frame on
    # a template does not change while it is held
    held = tracked[1:] & (B[1:] > 0)
    assert np.array_equal(bits(TM[1:][held]), bits(TM[:-1][held]))
    # every other feature-frame is the plain tracker's until the first drift loss differs the lists
    assert (E[tested] >= 0).all()


@pytest.mark.parametrize("seed", ds.SEEDS)
def test_entry_status_resets_the_slot(seed):
    """A slot entering with val > 0 (fresh) or val < 0 (lost) has age 0 afterwards, or 1 if it was tracked."""
    fr = scene(seed)
    s = ds.Shim()
    x, y, v = (np.array(a) for a in placed_list())
    n = len(x)
    tmpl, age = np.full((n, ds.NPX), 7.0, F32), np.full(n, 3, np.int32)
    v[0::3] = 5
    v[1::3] = -3
    keep = (x.copy(), y.copy())
    err = np.zeros(n, F32)
    s.track_drift(fr[0], fr[1], x, y, v, ds.MAX_RESIDUE, 0, tmpl, age, err)
    s.close()
    fresh, lost, held = np.arange(n) % 3 == 0, np.arange(n) % 3 == 1, np.arange(n) % 3 == 2
    assert (v[lost] == -3).all() and (age[lost] == 0).all() and same((x[lost], y[lost]), (keep[0][lost], keep[1][lost]))
    assert np.array_equal(age[fresh], (v[fresh] == 0).astype(np.int32)) and (v[fresh] == 0).sum() >= 40
    assert (err[fresh | lost] == -1.0).all()
    # the held slots were tested against the planted template (all 7.0): far off, so every tracked one is lost
    assert (err[held & (v == ds.DRIFTED)] > ds.MAX_RESIDUE).all() and (v[held] != 0).all()
    assert (v[held] == ds.DRIFTED).sum() >= 40 and (age[held] == 0).all()
    assert (tmpl[fresh & (v == 0)] != 7.0).any(axis=1).all() and (tmpl[lost] == 7.0).all()


@pytest.mark.parametrize("seed", ds.SEEDS)
def test_err_row_marks_the_tests(seed):
    for max_age in ds.AGES:
        X, Y, V, E, AGE, TM, B, _ = ds.placed_table(seed, max_age)
        prev = np.concatenate([placed_list()[2][None], V[:-1]])
        ran = (prev == 0) & (B > 0) & ((V == 0) | (V == ds.DRIFTED))
        assert np.array_equal(E == -1.0, ~ran) and ran.sum() >= 300
