"""The CPU side of what KLT_HIP_FAST is held to (tests/sum_scenes.py): the
statement of the window sums equals the oracle in the reference's order, the
bound B in tests/golden/fast_sums_160x120.json is what the float orders give,
every legitimate float32 order passes `accept`, and the mistakes a fast sum can
make are refused by it.

What `accept` cannot see is printed with its measured share and not asserted:
a mutant of the residue sum alone (it shows only in val, next to max_residue).
"""
from __future__ import annotations

import pytest

import motion_scenes as ms
import sum_scenes as ss

NAMES = list(ss.CONFIGS)
_measured: dict = {}


def measured(name):
    if name not in _measured:
        _measured[name] = ss.measure(name)
    return _measured[name]


def test_the_fixture_lists_the_configurations():
    fx = ss.fixture()
    assert list(fx["configs"]) == NAMES
    assert fx["max_share"] == ss.MAX_SHARE and fx["max_order_share"] == ss.MAX_ORDER_SHARE
    for base, _ in ss.GPU_VARIANTS.values():
        assert base in ss.CONFIGS
    # every window with lighting_insensitive 0 and 1
    for w, (ww, wh) in ss.WINDOWS.items():
        for li in (0, 1):
            cfg = ss.CONFIGS[w + ("_li" if li else "")]
            assert (cfg["window_width"], cfg["window_height"], cfg["lighting_insensitive"]) == (ww, wh, li)


@pytest.mark.parametrize("name", NAMES)
def test_seq_equals_orc_track(name):
    """SEQ -- float sums in the reference's order -- is the oracle bit for bit."""
    a, b = ss.run_table(name, ss.SEQ), ss.run_table(name, ss.SEQ, plain=True)
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes(), name


def test_seq_equals_the_oracle_library(oracle):
    """... and so is the shim's copy of the oracle the library the GPU tests compare with."""
    for name, mine in (("default", "w7"), ("lighting", "w7_li"), ("win9", "w9"), ("one_level", "w7_one_level")):
        want = ms.oracle_placed(oracle, 7, name)
        for p, q in zip(ss.run_table(mine, ss.SEQ), want):
            assert p.tobytes() == q.tobytes(), name


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    c = ss.check_conditions(name)
    assert c == ss.fixture()["configs"][name]["conditions"]
    if name in ss.DEGENERATE:
        assert c["tracked"] == 0 and c["losses"]["OOB"] == 251   # the whole placed list leaves in frame 1
    if name in ss.TWO_LOSSES:
        assert c["losses"]["MAX_ITERATIONS"] == 0 and c["losses"]["SMALL_DET"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_wide_replays_to_itself(name):
    """The replay along the WIDE table is that table: nothing else differs."""
    f = ss.figures(name, ss.run_table(name, ss.WIDE), B=0)
    assert f["compared"] >= 251 and f["disagree"] == 0 and f["max"] == 0, (name, f)


@pytest.mark.parametrize("name", NAMES)
def test_regenerated_figures_equal_the_fixture(name):
    m, fx = measured(name), ss.fixture()["configs"][name]
    assert m["B"] == fx["B"] == ss.bound(fx["orders"]) and m["B"] >= 4
    assert m == fx, name


@pytest.mark.parametrize("name", NAMES)
def test_every_float_order_passes(name):
    m = measured(name)
    for order in ss.ORDERS:
        f = m["orders"][order]
        print(f"{name} {order}: {f}")
        assert f["compared"] >= 251
        assert f["share"] <= ss.MAX_ORDER_SHARE, (name, order, f)
    ok, f = ss.accept(name, ss.run_table(name, *ss.ORDERS["tree"]), m["B"])
    assert ok and f == m["orders"]["tree"]


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ss.DEGENERATE])
def test_mutants_are_refused(name):
    m = measured(name)
    cases = ss.mutant_cases(name)
    assert ("c_leak", "all") in cases and (("d_drop_slot", "G") in cases) == (ss.npx_of(name) > 64)
    assert (("c_leak", "moments") in cases) == bool(ss.CONFIGS[name].get("lighting_insensitive", 0))
    for mutant, group in cases:
        share = m["mutants"][f"{mutant}/{group}"]
        required = ss.must_fail(name, mutant, group)
        print(f"{name} {mutant}/{group}: share {share:.4f}" + ("" if required else "  (recorded, not required)"))
        if required:
            assert share > ss.MAX_SHARE, (name, mutant, group, share)
    ok, f = ss.accept(name, ss.run_table(name, ss.LEAK, 0, ss.GROUPS["e"]), m["B"])
    assert not ok and f["share"] == m["mutants"]["c_leak/e"]
