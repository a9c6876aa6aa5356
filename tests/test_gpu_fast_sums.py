"""KLT_HIP_FAST held to its contract at every window geometry, and the exact
mode's multi-pixel-per-lane and lighting-insensitive sums held to the oracle.

KLT_HIP_FAST (include/klt_hip.h): each window sum is a float32 sum of the
reference's terms in an unspecified order, everything else as in
KLT_HIP_EXACT.  tests/sum_scenes.py states that on the CPU: a table is replayed
one frame at a time against the tracker with float64 sums, and accepted when at
most 0.5 % of the compared cells differ in status or lie more than B ulps from
it.  B per configuration is measured on the CPU from float32 sums in seven
orders (tests/golden/fast_sums_160x120.json; tests/test_fast_sums_host.py holds
the fixture, the orders and the mutants `accept` must refuse).  No table here
is compared with another table.

Every fast case prints its figures (compared cells, mismatches, p99 and max of
d) and, where KLT_FIGURES_DIR names a directory, writes them there as
fast_sums_<case>.json.

Exact mode is compared bit for bit with the oracle's per-frame loop.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest

import motion_scenes as ms
import sum_scenes as ss
from kltabi import arrays_to_fl, fl_to_arrays, u8ptr
from test_gpu_motion import assert_rows
from test_gpu_multi import Dev
from test_gpu_replace import ft_arrays

pytestmark = pytest.mark.gpu

FAST = 1
T7_FAST = (b"kltdev::k_track7<false, true, 2, true, true>", b"kltdev::k_track7_hook<2, true>",
           b"kltdev::k_track7<false, true, 2, true>")
GENERIC = b"kltdev::k_track_frames_g"


def held(case, name, table, start=None):
    """`accept` on a fast table with the configuration's B; the figures are kept."""
    ss.check_conditions(name)
    B = ss.B_of(name)
    ok, f = ss.accept(name, table, B, start)
    f = dict(f, B=B, config=name)
    print(f"\nfast sums {case}: {json.dumps(f)}")
    out = os.environ.get("KLT_FIGURES_DIR")
    if out and Path(out).is_dir():
        (Path(out) / f"fast_sums_{case}.json").write_text(json.dumps(f, indent=1) + "\n")
    assert ok, (case, f)
    return f


def batched(gpu, name, reduction, hook=None, chunk=4, calls=None):
    """The placed list on the configuration's scene through klt_hip_frames_begin +
    klt_hip_track_frames, the reduction set on the track descriptor."""
    d = Dev(gpu, setup=ss.tc_setup(gpu, name))
    if hook:
        d.ok(getattr(gpu, hook[0])(d.ctx, hook[1]), hook[0])
    d.td.reduction = reduction
    out = d.single(ss.frames_of(name), ms.placed_list(), chunk=chunk, calls=calls)
    kernel, nlevels = d.kernel(), d.pd.nlevels
    d.close()
    return out, kernel, nlevels


# ---------------------------------------------------------------------------
# a. every window geometry, lighting-insensitive or not, through the batched call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ss.CONFIGS))
def test_fast_batched(gpu, name):
    out, kernel, nlevels = batched(gpu, name, FAST)
    assert nlevels == ss.params(name).nPyramidLevels
    if name == "w7":   # the default: k_track7's fast instance; everything else the generic tracker's tree sums
        assert kernel in T7_FAST, kernel
    else:
        assert kernel == GENERIC, kernel
    held(name, name, out)
    for f, row in zip(out[3:], (a[-1] for a in out[:3])):
        assert f.tobytes() == row.tobytes(), "the final list is not the last row"


@pytest.mark.parametrize("case", list(ss.GPU_VARIANTS))
def test_fast_batched_other_kernels(gpu, case):
    """7x7, two levels, away from k_track7: the generic tracker without and with the lane patch."""
    name, hook = ss.GPU_VARIANTS[case]
    out, kernel, _ = batched(gpu, name, FAST, hook=hook)
    assert kernel == GENERIC, kernel
    held(case, name, out)


# ---------------------------------------------------------------------------
# b. k_track7's fast instances under every schedule
# ---------------------------------------------------------------------------
T7_CASES = {
    "w7_chunk1": dict(chunk=1), "w7_chunk64": dict(chunk=64), "w7_calls_3_4_6": dict(calls=[3, 4, 6]),
    "w7_lazy_off": dict(hook=("klt_hip_set_lazy_grad", 0)), "w7_merge_off": dict(hook=("klt_hip_set_track_merge", 0)),
    "w7_input_order": dict(hook=("klt_hip_set_track_order", 1)),
}


@pytest.mark.parametrize("case", list(T7_CASES))
def test_fast_track7_schedules(gpu, case):
    out, kernel, nlevels = batched(gpu, "w7", FAST, **T7_CASES[case])
    assert nlevels == 2 and kernel in T7_FAST, kernel
    held(case, "w7", out)


# ---------------------------------------------------------------------------
# c. the klt.h surface with klt_amd_set_reduction
# ---------------------------------------------------------------------------
def klt_context(gpu, name, sequential):
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1 if sequential else 0
    tc.contents.writeInternalImages = 0
    tc.contents.affineConsistencyCheck = -1
    ss.tc_setup(gpu, name)(tc.contents)
    gpu.klt_amd_set_reduction(tc, FAST)
    fl = gpu.KLTCreateFeatureList(len(ms.placed_list()[0]))
    arrays_to_fl(fl, *ms.placed_list())
    return tc, fl


@pytest.mark.parametrize("name", ["w7", "w9_li"])
@pytest.mark.parametrize("sequential", [True, False])
def test_fast_klt_track_features_loop(gpu, name, sequential):
    fr = ss.frames_of(name)
    h, w = fr[0].shape
    tc, fl = klt_context(gpu, name, sequential)
    rows = []
    for i in range(1, len(fr)):
        gpu.KLTTrackFeatures(tc, u8ptr(fr[i - 1]), u8ptr(fr[i]), w, h, fl)
        rows.append(fl_to_arrays(fl))
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    table = tuple(np.stack([r[k] for r in rows]) for k in range(3))
    held(f"{name}_klt_loop_{'sequential' if sequential else 'pairs'}", name, table)


def test_fast_klt_track_sequence(gpu):
    fr = ss.frames_of("w7")
    h, w = fr[0].shape
    n = len(ms.placed_list()[0])
    tc, fl = klt_context(gpu, "w7", True)
    ft = gpu.KLTCreateFeatureTable(ss.T, n)
    arr = (C.POINTER(C.c_ubyte) * len(fr))(*[u8ptr(f) for f in fr])
    gpu.KLTTrackSequence(tc, arr, len(fr), w, h, fl, ft, 0)
    table = ft_arrays(ft, n, 0, ss.T)
    last = fl_to_arrays(fl)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    held("w7_klt_track_sequence", "w7", table)
    for f, row in zip(last, (a[-1] for a in table)):
        assert f.tobytes() == row.tobytes(), "the final list is not the last row"


# ---------------------------------------------------------------------------
# d. exact mode: every window, lighting-insensitive or not, bit for bit
# ---------------------------------------------------------------------------
# test_gpu_motion holds 7x7, 7x7 lighting-insensitive, 9x9 and the one-level pyramid already
EXACT = [n for n in ss.CONFIGS if n not in ("w7", "w7_li", "w9", "w7_one_level")]


@pytest.mark.parametrize("name", EXACT)
def test_exact_batched(gpu, oracle, name):
    ss.check_conditions(name)
    want = ms.oracle_table(oracle, ("sums", name), ss.frames_of(name), ms.placed_list(), ss.params(name, oracle))
    for p, q in zip(want, ss.run_table(name, ss.SEQ)):
        assert p.tobytes() == q.tobytes()   # the conditions were asserted on this table
    out, kernel, _ = batched(gpu, name, 0)
    if ss.npx_of(name) == 49:   # 7x7 at other depths: k_track7 on planes
        assert kernel.startswith(b"kltdev::k_track7<"), kernel
    else:
        assert kernel == GENERIC, kernel
    assert_rows(out, want, name, final=out[3:])


def test_a_reused_context_lays_its_banks_out_again(gpu, oracle):
    """A tracking context's device context is kept for the next tracking context.
    Three levels of subsampling 8 and then of subsampling 2 have the same depth
    and the same level 0: banks laid out for the first (level 1: 20x15) must not
    pass for the second (80x60), where they would be written past their end and
    every feature would leave the 20x15 level."""
    for name in ("w7_three_levels_sr120", "w7_three_levels"):
        want = ms.oracle_table(oracle, ("sums", name), ss.frames_of(name), ms.placed_list(), ss.params(name, oracle))
        out, _, nlevels = batched(gpu, name, 0)
        assert nlevels == 3
        assert_rows(out, want, name, final=out[3:])
    assert (want[2] == 0).sum() >= ss.MIN_TRACKED
