"""The CPU statement of the region mask (tests/native/mask_oracle.c) held to
the oracle, and the conditions on its tables that the GPU comparisons of
tests/test_gpu_mask_*.py rest on (asserted there again before any comparison).

Measured on motion_scenes.scene (160x120, placed_list()'s 251 features, 13
tracked frames) with mask_scenes.scene_mask():

                                              seed 7    seed 8
    MASKED slots                                40        40
    of them at frame 1                          25        25
    of them walking in over frames 2-13         15        15
    of them LARGE_RESIDUE before the mask test   8         7
    alive at the end (unmasked)                 61 (73)   65 (78)

mask_scenes.FLOORS are about half of those figures.  No feature is lost to the
mask with KLT_MAX_ITERATIONS pending on these scenes: mask_scenes.maxit_table
makes one by zeroing the pixel under such a feature's final position.
"""
from __future__ import annotations

import numpy as np
import pytest

import mask_scenes as ms
from kltabi import OracleTracker, load_dataset
from motion_scenes import F32, H, LARGE_RESIDUE, MAX_ITERATIONS, NOT_FOUND, OOB, SMALL_DET, W, placed_list, scene


def bits(a):
    return np.asarray(a).view(np.int32)


def same(a, b):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))


ALL_ALLOWED = np.ones((H, W), np.uint8)
ALL_MASKED = np.zeros((H, W), np.uint8)


@pytest.mark.parametrize("seed", ms.SEEDS)
@pytest.mark.parametrize("mask", [None, ALL_ALLOWED], ids=["null", "all_allowed"])
def test_no_mask_is_the_oracle(oracle, seed, mask):
    """orc_select_mask, orc_replace_mask and orc_track_mask give orc_select,
    orc_replace and orc_track bit for bit."""
    fr = scene(seed)
    o, s = OracleTracker(oracle), ms.Shim()
    o.params.sequentialMode = 1
    oracle.orc_set_params(o.h, o.params)
    want = o.select(fr[0], 50)
    got = s.select_mask(fr[0], 50, mask)
    assert same(got, want) and (want[2] > 0).all()
    for i in range(1, 7):
        o.track(fr[i - 1], fr[i], *want)
        s.track_mask(fr[i - 1], fr[i], *got, mask)
        assert same(got, want), i
        if i % 3 == 0:
            lost = int((want[2] < 0).sum())
            o.replace(fr[i], *want)
            s.replace_mask(fr[i], *got, mask)
            assert same(got, want), i
            assert lost > int((want[2] < 0).sum())  # something was replaced
    o.close()
    s.close()


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_all_masked(seed):
    fr = scene(seed)
    s = ms.Shim()
    x, y, v = s.select_mask(fr[0], 50, ALL_MASKED)
    assert (v == NOT_FOUND).all() and (x == -1).all() and (y == -1).all()
    # replacement: live features stay, lost slots stay lost
    x, y, v = (a.copy() for a in placed_list())
    v[::2] = -3
    keep = (x.copy(), y.copy(), v.copy())
    s.replace_mask(fr[0], x, y, v, ALL_MASKED)
    live = keep[2] >= 0
    assert same((x[live], y[live], v[live]), tuple(a[live] for a in keep)) and (v[~live] == NOT_FOUND).all()
    s.close()
    # tracking: every live feature is lost by frame 1, to the mask unless the border or a small determinant took it
    t = ms.shim_table(("all_masked", seed), fr[:2], placed_list(), track_mask=ALL_MASKED)
    V, PRE = t[2][0], t[3][0]
    assert (V < 0).all()
    assert set(V[(PRE != OOB) & (PRE != SMALL_DET)]) == {ms.MASKED}
    assert np.array_equal(V[(PRE == OOB) | (PRE == SMALL_DET)], PRE[(PRE == OOB) | (PRE == SMALL_DET)])
    assert (V == ms.MASKED).sum() > 200


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_scene_conditions(seed):
    c = ms.assert_scene_conditions(seed)
    m = ms.MEASURED[seed]
    assert {k: c[k] for k in ("masked", "frame1", "later", "pre_large_residue", "alive")} == \
        {k: m[k] for k in ("masked", "frame1", "later", "pre_large_residue", "alive")}
    assert c["pre_max_iterations"] == 0
    assert ms.counts(ms.placed_table(seed, masked=False))["alive"] == m["alive_unmasked"]
    # the rule, on the table: a masked feature's pre-mask position is on a zero byte, inside the border, and its
    # pre-mask status is anything but OOB and SMALL_DET; every other tracked feature-frame keeps the oracle's status
    X, Y, V, PRE, PX, PY = ms.placed_table(seed)
    mask = ms.scene_mask()
    tracked = PRE != 7
    on_zero = np.zeros_like(tracked)
    ok = tracked & (PRE != OOB) & (PRE != SMALL_DET)
    on_zero[ok] = mask[PY[ok].astype(int), PX[ok].astype(int)] == 0
    assert np.array_equal(V == ms.MASKED, on_zero | ((V == ms.MASKED) & ~tracked))
    assert np.array_equal(V[tracked & ~on_zero], PRE[tracked & ~on_zero])
    assert set(PRE[on_zero]) <= {0, LARGE_RESIDUE, MAX_ITERATIONS}
    assert (X[V == ms.MASKED] == -1).all() and (Y[V == ms.MASKED] == -1).all()
    # a masked feature is lost from that frame on
    for r, k in np.argwhere(V == ms.MASKED):
        assert (V[r:, k] == ms.MASKED).all()


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_max_iterations_precedence_case(seed):
    m, t, (row, k) = ms.maxit_table(seed)
    assert t[2][row, k] == ms.MASKED and t[3][row, k] == MAX_ITERATIONS
    assert ms.counts(t)["pre_max_iterations"] >= 1
    assert ms.placed_table(seed)[2][row, k] == MAX_ITERATIONS  # without that pixel: the oracle's status


def test_pitch_and_padding():
    """A mask with pitch > ncols whose padding holds the opposite value reads as the tight one."""
    fr = scene(7)
    s = ms.Shim()
    tight, wide = ms.scene_mask(), ms.scene_mask(pitch=W + 37, pad=0)
    assert same(s.select_mask(fr[0], 50, wide), s.select_mask(fr[0], 50, tight))
    inv_t = (1 - ms.scene_mask()).astype(np.uint8)
    inv_w = np.ones((H, W + 5), np.uint8)
    inv_w[:, :W] = inv_t
    a, b = s.select_mask(fr[0], 50, inv_w), s.select_mask(fr[0], 50, inv_t)
    assert same(a, b) and (a[2] > 0).sum() >= 3
    s.close()
    t = ms.shim_table(("wide", 7), fr, placed_list(), track_mask=wide)
    assert same(t[:3], ms.placed_table(7)[:3])


def test_selection_avoids_the_mask():
    """images_provided/img0 at 320x240, 150 features: the mask is built from the
    unmasked selection so that at least a quarter of it lies on masked pixels."""
    img = load_dataset(n=1)[0]
    mask, plain = img0_mask(img)
    s = ms.Shim()
    x, y, v = s.select_mask(img, 150, mask)
    s.close()
    got = v > 0
    assert got.sum() >= 100 and (mask[y[got].astype(int), x[got].astype(int)] != 0).all()
    assert not same((x, y, v), plain)


_img0: dict = {}


def img0_mask(img):
    """Zero squares of 9x9 around every third feature of the unmasked selection
    (and a zero bar along the left edge of the selectable area)."""
    if "m" not in _img0:
        s = ms.Shim()
        plain = s.select_mask(img, 150, None)
        s.close()
        h, w = img.shape
        m = np.ones((h, w), np.uint8)
        x, y, v = plain
        for k in range(0, 150, 3):
            if v[k] > 0:
                m[max(int(y[k]) - 4, 0):int(y[k]) + 5, max(int(x[k]) - 4, 0):int(x[k]) + 5] = 0
        m[:, :40] = 0
        ok = v > 0
        hit = (m[y[ok].astype(int), x[ok].astype(int)] == 0).sum()
        assert hit * 4 >= ok.sum() >= 140, (hit, ok.sum())
        m.setflags(write=False)
        _img0["m"] = (m, tuple(a.copy() for a in plain))
    return _img0["m"]
