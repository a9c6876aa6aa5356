"""The CPU statement of the motion prior (tests/native/predict_oracle.c) held
to the oracle, and the conditions on its tables that the GPU comparisons of
tests/test_gpu_predict.py rest on (asserted there again before any comparison).

Measured on the frames of predict_scenes.scene (oracle tables, 143-point
lattice, 13 tracked frames):

    seed   alive with the prior   alive without   feature-frames entered with a nonzero state
    7      132 (11 lost, all OOB)   34 (98 LARGE_RESIDUE, 11 OOB)   1639
    8      132 (11 lost, all OOB)  103 (30 LARGE_RESIDUE, 10 OOB)   1639

FLOORS are what the comparisons need, below those figures: a changed input
cannot quietly turn the scene into one that any start follows.
"""
from __future__ import annotations

import numpy as np
import pytest

import predict_scenes as ps
from motion_scenes import F32, LARGE_RESIDUE, OOB

FLOORS = dict(alive_with=120, alive_without=110, nonzero=1000)
MEASURED = {7: (132, 34, 1639), 8: (132, 103, 1639)}


def bits(a):
    return np.asarray(a).view(np.int32)


def assert_scene_conditions(seed):
    """The floors, on the shim's tables."""
    a, b = ps.shim_lattice(seed, True), ps.shim_lattice(seed, False)
    assert ps.alive(a[2]) >= FLOORS["alive_with"]
    assert ps.alive(b[2]) <= FLOORS["alive_without"]
    assert int(a[5].sum()) >= FLOORS["nonzero"]


def first_frame(seed, state, predict=True):
    fr = ps.scene(seed)[:2]
    return ps.shim_table(("first", seed, predict, None if state is None else tuple(bits(s).tobytes() for s in state)),
                         fr, ps.lattice(), state=state, predict=predict)


def seeded(value_x, value_y, n=143):
    """Every third feature seeded, the others zero."""
    vx, vy = np.zeros(n, F32), np.zeros(n, F32)
    vx[::3], vy[::3] = value_x, value_y
    return vx, vy


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_zero_state_first_frame_is_the_oracle(oracle, seed):
    from kltabi import OracleTracker
    fr = ps.scene(seed)
    o = OracleTracker(oracle)
    x, y, v = (a.copy() for a in ps.lattice())
    o.track(fr[0], fr[1], x, y, v)
    o.close()
    X, Y, V = first_frame(seed, None)[:3]
    assert np.array_equal(V[0], v) and np.array_equal(bits(X[0]), bits(x)) and np.array_equal(bits(Y[0]), bits(y))
    # ... and the shim's own orc_track (the included oracle) is that oracle
    X, Y, V = first_frame(seed, None, predict=False)[:3]
    assert np.array_equal(V[0], v) and np.array_equal(bits(X[0]), bits(x)) and np.array_equal(bits(Y[0]), bits(y))


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_scene_conditions(seed):
    assert_scene_conditions(seed)
    a, b = ps.shim_lattice(seed, True), ps.shim_lattice(seed, False)
    assert (ps.alive(a[2]), ps.alive(b[2]), int(a[5].sum())) == MEASURED[seed]
    # what the prior saves was lost to the residue; what it loses left the border
    assert set(a[2][-1][a[2][-1] < 0]) == {OOB}
    assert int((b[2][-1] == LARGE_RESIDUE).sum()) == {7: 98, 8: 30}[seed]
    # the state is the displacement: two float subtractions of the rows
    x0, y0, _ = ps.lattice()
    X, Y, V, VX, VY = a[:5]
    for j in range(ps.T):
        px, py = (x0, y0) if j == 0 else (X[j - 1], Y[j - 1])
        ok = V[j] == 0
        assert np.array_equal(bits(VX[j][ok]), bits((X[j] - px)[ok])) and np.array_equal(bits(VY[j][ok]), bits((Y[j] - py)[ok]))
        assert not VX[j][~ok].any() and not VY[j][~ok].any()
    assert float(np.abs(VX).max()) > 13.0  # steps the zero start does not follow


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("big", [1e4, np.inf])
def test_huge_state_takes_the_unpredicted_start(seed, big):
    """Rule 3: the start's window is outside the coarsest level."""
    plain = first_frame(seed, None, predict=False)
    got = first_frame(seed, seeded(big, -big))
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(plain[k]))


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_nan_state_takes_the_unpredicted_start(seed):
    """The inside test fails on a NaN (an outside test would pass it on)."""
    plain = first_frame(seed, None, predict=False)
    for state in (seeded(np.nan, 0.0), seeded(0.0, np.nan), seeded(np.nan, np.nan)):
        got = first_frame(seed, state)
        for k in range(3):
            assert np.array_equal(bits(got[k]), bits(plain[k]))
        assert not np.isnan(got[3]).any() and not np.isnan(got[4]).any()


def replace_case(seed):
    """The replacement case of the GPU tests: the list orc_select gives on
    frame 0 (val > 0: rule 1), orc_replace after every third frame."""
    fr = ps.scene(seed)
    o = ps.Shim()
    start = o.select(fr[0], 120)
    o.close()
    return start, ps.shim_table(("replace", seed), fr, start, every=3)


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_replacement_case_conditions(seed):
    start, (X, Y, V, VX, VY, NZ) = replace_case(seed)
    assert (start[2] > 0).all()
    assert not NZ[0].any() and NZ[1:].any()  # fresh features start from zero, tracked ones carry a state
    # a slot lost by frame 3, 6 or 9, filled there, and tracked by the frame after
    refilled = 0
    for j in (2, 5, 8):
        filled = V[j] > 0
        assert not VX[j][filled].any() and not VY[j][filled].any()  # lost by the tracker: no state
        refilled += int((filled & (V[j + 1] == 0)).sum())
    assert refilled >= 1
