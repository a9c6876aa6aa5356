"""The CPU statement of the frame prior (tests/native/frame_prior_oracle.c)
held to the oracle, and the conditions on its tables that comparisons of a
device implementation rest on (assert_scene_conditions, replace_case and
rule3_rows are written to be asserted there again before any comparison).

Measured on the frames of frame_prior_scenes.scene (shim tables, 143-point
lattice, 13 tracked frames; alive after each frame, then the losses at the end):

    start of the search            seed 7                          seed 8
    zero motion (orc_track)        27, then 0 (143 LARGE_RESIDUE)  48, 12, 10, 5, 5, 2 ... 0 (143 LARGE_RESIDUE)
    last displacement              27, then 0 (139 LR, 4 OOB)      48, then 0 (143 LARGE_RESIDUE)
    the true rows                  143 on every frame              143 on every frame
    projective rows                143 on every frame              143 on every frame
    biased rows (13 px, every 3rd) 47 (95 LARGE_RESIDUE, 1 OOB)    55 (88 LARGE_RESIDUE)

and with the translation off by (+11, -11) px on every third frame 83 / 102,
by (+6, -6) px on every third frame or on every frame 143 / 143.

FLOORS are what the comparisons need, away from those figures: a changed input
cannot quietly turn the scene into one that any start follows, or the biased
table into one that loses nothing.
"""
from __future__ import annotations

import numpy as np
import pytest

import frame_prior_scenes as fs
from motion_scenes import F32, LARGE_RESIDUE, OOB

FLOORS = dict(alive_true=135, alive_plain=10, alive_last=10, biased=(20, 100), biased_residue=30)
MEASURED = {  # alive at the end: plain, last motion, true, projective, biased; the biased table's LARGE_RESIDUE, OOB
    7: (0, 0, 143, 143, 47, 95, 1),
    8: (0, 0, 143, 143, 55, 88, 0),
}


def bits(a):
    return np.asarray(a).view(np.int32)


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def assert_scene_conditions(seed):
    """The floors, on the shim's tables."""
    assert fs.alive(fs.shim_prior(seed, "true")[2]) >= FLOORS["alive_true"]
    assert fs.alive(fs.shim_prior(seed, "projective")[2]) >= FLOORS["alive_true"]
    assert fs.alive(fs.shim_plain(seed)[2]) <= FLOORS["alive_plain"]
    assert fs.alive(fs.shim_last_motion(seed)[2]) <= FLOORS["alive_last"]
    V = fs.shim_prior(seed, "biased")[2]
    lo, hi = FLOORS["biased"]
    assert lo <= fs.alive(V) <= hi
    assert int((V[-1] == LARGE_RESIDUE).sum()) >= FLOORS["biased_residue"]
    assert any(int((fs.shim_prior(s, "biased")[2][-1] == OOB).sum()) >= 1 for s in fs.SEEDS)


def first_frame(seed, row):
    """Frame 1 of the lattice under one row (None: orc_track)."""
    fr = fs.scene(seed)[:2]
    if row is None:
        return fs.shim_table(("first", seed, None), fr, fs.lattice())
    row = np.asarray(row, F32)
    return fs.shim_table(("first", seed, row.tobytes()), fr, fs.lattice(), rows=row[None])


def rule3_rows():
    """Rows whose start is outside every level, or no number: NaN in each part,
    +-inf, all zeros (w = 0: 0/0), w = 0 over a finite numerator (+-inf), a huge
    translation."""
    t = fs.rows_of("true")[0]
    out = {}
    for name, k, val in (("nan_m0", 0, np.nan), ("nan_m5", 5, np.nan), ("nan_m8", 8, np.nan), ("inf_m2", 2, np.inf),
                         ("minus_inf_m5", 5, -np.inf), ("inf_m8", 8, np.inf), ("w_zero", 8, 0.0), ("huge_x", 2, 1e6),
                         ("huge_negative_y", 5, -1e6)):
        r = np.array(t, F32)
        r[k] = val
        out[name] = r
    out["all_zero"] = np.zeros(9, F32)
    return out


@pytest.mark.parametrize("seed", fs.SEEDS)
def test_identity_rows_are_the_oracle(oracle, seed):
    """Bit for bit on every frame: against the shim's own orc_track, and
    against the oracle library the other tests use."""
    from kltabi import OracleTracker
    fr = fs.scene(seed)
    got = fs.shim_table(("identity", seed), fr, fs.lattice(), rows=fs.identity_rows())
    assert same(got, fs.shim_plain(seed))
    o = OracleTracker(oracle)
    x, y, v = (a.copy() for a in fs.lattice())
    for i in range(1, fs.NFRAMES):
        o.track(fr[i - 1], fr[i], x, y, v)
        assert same((x, y, v), tuple(g[i - 1] for g in got)), i
    o.close()


@pytest.mark.parametrize("seed", fs.SEEDS)
@pytest.mark.parametrize("name", sorted(rule3_rows()))
def test_rows_without_a_start_take_the_plain_start(seed, name):
    """Rule 3: the first frame is the plain tracker's."""
    assert same(first_frame(seed, rule3_rows()[name]), first_frame(seed, None))
    # ... which the true row's is not: the rule decides something here
    assert not same(first_frame(seed, fs.rows_of("true")[0]), first_frame(seed, None))


@pytest.mark.parametrize("seed", fs.SEEDS)
def test_scene_conditions(seed):
    assert_scene_conditions(seed)
    Vb = fs.shim_prior(seed, "biased")[2]
    got = (fs.alive(fs.shim_plain(seed)[2]), fs.alive(fs.shim_last_motion(seed)[2]),
           fs.alive(fs.shim_prior(seed, "true")[2]), fs.alive(fs.shim_prior(seed, "projective")[2]), fs.alive(Vb),
           int((Vb[-1] == LARGE_RESIDUE).sum()), int((Vb[-1] == OOB).sum()))
    assert got == MEASURED[seed]
    # both existing starts have lost everything by the second frame (seed 8's zero start: by the eleventh)
    assert fs.alive(fs.shim_last_motion(seed)[2][:2]) == 0
    assert fs.alive(fs.shim_plain(seed)[2][:{7: 2, 8: 11}[seed]]) == 0
    # the true rows keep every feature on every frame, w == 1 or not
    for name in ("true", "projective"):
        assert (fs.shim_prior(seed, name)[2] == 0).all()
    # the projective rows do start elsewhere: their results differ from the true rows'
    assert not same(fs.shim_prior(seed, "projective")[:2], fs.shim_prior(seed, "true")[:2])
    # the biased rows lose features on the frames they are off, and only there
    lost = [int(((Vb[j] < 0) & ((Vb[j - 1] == 0) if j else True)).sum()) for j in range(fs.T)]
    assert lost[2] >= 50 and not lost[0] and not lost[1]


def test_rows_are_the_frame_to_frame_transform():
    """M_t takes a pixel of frame t - 1 to the pixel of frame t that shows the
    same texture point (to float32 rounding of the row)."""
    M = fs.rows_of("true").astype(np.float64)
    x, y, _ = fs.lattice()
    x, y = x.astype(np.float64), y.astype(np.float64)
    for t in range(1, fs.NFRAMES):
        m = M[t - 1]
        assert (m[6], m[7], m[8]) == (0.0, 0.0, 1.0)
        gx, gy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        a, b, c, d, e, f = fs.to_texture(t - 1)
        pa, pb, pc, pd, pe, pf = fs.to_texture(t)
        assert np.abs((pa * gx + pb * gy + pc) - (a * x + b * y + c)).max() < 1e-3
        assert np.abs((pd * gx + pe * gy + pf) - (d * x + e * y + f)).max() < 1e-3
    steps = np.abs(M[:, 2])
    assert steps.min() > 13.0 and steps.max() < 32.0  # what neither existing start follows
    B = fs.rows_of("biased")
    assert np.array_equal(np.flatnonzero((B != fs.rows_of("true")).any(axis=1)), [2, 5, 8, 11])


def replace_case(seed):
    """The replacement case: the list orc_select gives on frame 0 (val > 0),
    orc_replace after every third frame, the biased rows."""
    fr = fs.scene(seed)
    o = fs.Shim()
    start = o.select(fr[0], 120)
    o.close()
    return start, fs.shim_table(("replace", seed), fr, start, rows=fs.rows_of("biased"), every=3)


@pytest.mark.parametrize("seed", fs.SEEDS)
def test_replacement_case_conditions(seed):
    start, (X, Y, V) = replace_case(seed)
    assert (start[2] > 0).all()  # fresh from selection: tracked under the prior like any other slot
    # measured: 97 of the 120 tracked on frame 1 (both seeds; the rest leave the image with the shift), against
    # 36 (seed 7) and 46 (seed 8) from the zero start
    plain = fs.shim_table(("replace-plain", seed), fs.scene(seed)[:2], start)
    assert int((V[0] == 0).sum()) >= 80 and int((plain[2][0] == 0).sum()) <= 60
    # a slot lost by frame 3, 6 or 9, filled there, and tracked by the frame after
    # (measured: 53 + 61 + 58 and 48 + 58 + 53 of them)
    refilled = 0
    for j in (2, 5, 8):
        filled = V[j] > 0
        refilled += int((filled & (V[j + 1] == 0)).sum())
    assert refilled >= 20
