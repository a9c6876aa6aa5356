"""The processing order's balanced layout (klt_hip_order_slot), host only.

A tracker launch over n features hands XCD x the slots of segment x,
[min(x S, n), min((x + 1) S, n)) with S = 4 * xcd_per.  The layout gives every
segment its share of the live features, in band order, and fills it up with
lost ones, so that the waves that leave at once are spread over all eight
XCDs.  Checked here against a numpy restatement of the formula and for the
properties the tracker relies on: a permutation of the slots, no segment over
its capacity, equal shares, live ranks increasing through the segments."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

NS = [1, 4, 37, 2048, 2051, 5000, 20000]
XCDS, WAVES = 8, 4


def xcd_per_of(n):
    return ((n + WAVES - 1) // WAVES + XCDS - 1) // XCDS


def lives_of(n):
    return sorted({0, 1, n // 3, n - 1, n} & set(range(n + 1)))


def layout(n, xcd_per, n_live):
    """(slot of every live rank, slot of every lost rank, segment edges, live starts)"""
    S = WAVES * xcd_per
    edge = np.minimum(np.arange(XCDS + 1, dtype=np.int64) * S, n)
    B = n_live * edge // n
    live_x = np.diff(B)
    LB = np.concatenate([[0], np.cumsum(np.diff(edge) - live_x)])
    q = np.arange(n_live, dtype=np.int64)
    xq = np.searchsorted(B, q, side="right") - 1
    p = np.arange(n - n_live, dtype=np.int64)
    xp = np.searchsorted(LB, p, side="right") - 1
    return xq * S + (q - B[xq]), xp * S + live_x[xp] + (p - LB[xp]), edge, B


def slots(amd, n, xcd_per, n_live, lost):
    out = np.empty(n - n_live if lost else n_live, np.int64)
    s = C.c_int(-7)
    for r in range(len(out)):
        assert amd.klt_hip_order_slot(n, xcd_per, n_live, r, lost, C.byref(s)) == 0, (n, n_live, r, lost)
        out[r] = s.value
    return out


@pytest.mark.parametrize("n", NS)
def test_slots_equal_the_formula_and_keep_its_properties(amd, n):
    xp = xcd_per_of(n)
    S = WAVES * xp
    for n_live in lives_of(n):
        want_live, want_lost, edge, B = layout(n, xp, n_live)
        live, lost = slots(amd, n, xp, n_live, 0), slots(amd, n, xp, n_live, 1)
        assert np.array_equal(live, want_live), (n, n_live)
        assert np.array_equal(lost, want_lost), (n, n_live)
        # a permutation of 0..n-1
        assert np.array_equal(np.sort(np.concatenate([live, lost])), np.arange(n)), (n, n_live)
        # no segment overflows: every slot lies inside the segment it was given to
        for s in (live, lost):
            x = s // S
            assert (x < XCDS).all() and (s < edge[x + 1]).all() and (s >= edge[x]).all(), (n, n_live)
        # equal capacity, live counts within one of each other
        live_x = np.bincount(live // S, minlength=XCDS)
        assert np.array_equal(live_x, np.diff(B))
        cap = np.diff(edge)
        for c in np.unique(cap):
            assert np.ptp(live_x[cap == c]) <= 1, (n, n_live, live_x, cap)
        assert (live_x <= cap).all()
        # live ranks read segment by segment (slot order) are increasing, and
        # within a segment every live slot precedes every lost one
        assert (np.diff(live) > 0).all()
        assert (np.diff(lost) > 0).all()
        for x in range(XCDS):
            lv, lo = live[live // S == x], lost[lost // S == x]
            if len(lv) and len(lo):
                assert lv.max() < lo.min()


def test_arguments_out_of_range_are_refused(amd):
    s = C.c_int(-7)
    ok = lambda *a: amd.klt_hip_order_slot(*a, C.byref(s))  # noqa: E731
    assert ok(37, xcd_per_of(37), 12, 0, 0) == 0 and s.value == 0
    for bad in ((0, 1, 0, 0, 0), (37, 0, 12, 0, 0), (37, 1, 12, 0, 0),  # 8 segments of 4 slots < 37
                (37, 2, 38, 0, 0), (37, 2, -1, 0, 0), (37, 2, 12, 12, 0), (37, 2, 12, 25, 1), (37, 2, 12, -1, 1)):
        s.value = -7
        assert ok(*bad) == -1 and s.value == -7, bad
    assert amd.klt_hip_order_slot(37, 2, 12, 0, 0, None) == -1
