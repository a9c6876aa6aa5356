"""The affine consistency check inside the batched tracker launch
(klt_hip_set_frames_affine), CPU side: the fixtures
tests/golden/affine_batched_*.npz (the reference's outputs, written by
tests/golden/make_affine_batched.py) are reproduced by the oracle, they
exercise the stage, and the new entry points exist and check their arguments
without a device.  The GPU side is tests/test_gpu_affine_batched.py.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import pytest

from kltabi import GOLDEN, OracleTracker, TrackingContextRec, affine_setup

sys.path.insert(0, str(GOLDEN))
from make_affine_batched import BATCHED_CASES  # noqa: E402
from make_golden import affine_inputs  # noqa: E402
from test_affine import FIELDS, mismatches  # noqa: E402

CASES = {c[0]: c for c in BATCHED_CASES}
IDENT = np.array([1, 0, 0, 1], np.float32)


def golden(name):
    d = np.load(GOLDEN / f"{name}.npz")
    return tuple(d[k] for k in FIELDS)


def test_cases_are_the_issue_s():
    """Windows above the 256-pixel chunk (17, 23), below one wave (5), every
    mode, one lighting-insensitive: 100 features over the 10 provided frames."""
    got = sorted((kw["mode"], kw.get("window", 15), kw.get("li", 0)) for _, _, _, _, _, kw in BATCHED_CASES)
    assert got == [(0, 17, 1), (1, 5, 0), (2, 5, 0), (2, 17, 0), (2, 23, 0)]
    for _, data, n, nf, replace, kw in BATCHED_CASES:
        assert (data, n, nf, replace) == ("images_provided", 100, 10, False)
        if kw.get("window") in (17, 23) and kw["mode"] == 2:
            assert (kw["mdd"], kw["max_res"]) == (3.0, 20.0)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_fixture(oracle, name):
    _, data, n, nf, replace, kw = CASES[name]
    tc = TrackingContextRec()
    affine_setup(**kw)(tc)
    o = OracleTracker(oracle)
    o.params.lighting_insensitive = tc.lighting_insensitive
    got = o.harness_affine(affine_inputs(data), n, nf, tc, replace=replace)
    assert mismatches(got, golden(name)) == []


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_exercises_the_stage(name):
    """A GPU test must not pass on a stage that never ran: windows are held to
    the end, held windows are lost on the way, and A leaves the identity."""
    X, Y, V, A, H, K = golden(name)
    mode = CASES[name][5]["mode"]
    held = H[-1] == 1
    assert held.sum() >= 20
    lost_held = ((H[:-1] == 1) & (H[1:] == 0)).any(axis=0)
    assert lost_held.sum() >= 10
    if mode in (1, 2):
        assert np.abs(A[-1][held][:, 2:] - IDENT).max() > 0.02
    else:
        assert (A[:, :, 2:] == IDENT).all()
    assert (K[-1][held] != 0).all() and (K[-1][~held] == 0).all()


NEW_ENTRY_POINTS = ("klt_hip_set_frames_affine", "klt_hip_get_frames_affine", "klt_hip_set_affine_table",
                    "klt_hip_affine_state_put", "klt_hip_affine_state_get")


def test_entry_points_exported(amd):
    from kltamd.device import DEVICE_PROTOS
    for name in NEW_ENTRY_POINTS + ("klt_hip_affine_reserve", "klt_hip_affine_put", "klt_hip_affine_get",
                                    "klt_hip_track_affine", "klt_hip_track_frames_host"):
        assert hasattr(amd, name), name
        assert name in DEVICE_PROTOS, name


def test_header_declares_entry_points():
    from kltabi import ROOT
    text = (ROOT / "include" / "klt_hip.h").read_text()
    for name in NEW_ENTRY_POINTS:
        assert f"int {name}(" in text, name


def test_null_context_and_bad_arguments_fail_without_a_device(amd):
    from kltamd.device import AffineDesc
    tc = TrackingContextRec()
    affine_setup(mode=2)(tc)
    tc.min_determinant, tc.min_displacement, tc.step_factor = 0.01, 0.1, 1.0
    ad = AffineDesc.from_tc(tc)
    assert (ad.mode, ad.window_width, ad.window_height, ad.max_iterations) == (2, 15, 15, 10)
    buf = (C.c_float * 6)()
    st = (C.c_int * 1)()
    on = C.c_int(7)
    pa, ps = C.c_void_p(), C.c_void_p()
    assert amd.klt_hip_set_frames_affine(None, C.byref(ad), buf, st) == -1
    assert amd.klt_hip_set_frames_affine(None, None, None, None) == -1
    assert amd.klt_hip_get_frames_affine(None, C.byref(on)) == -1 and on.value == 7
    assert amd.klt_hip_set_affine_table(None, buf, st, 1) == -1
    assert amd.klt_hip_set_affine_table(None, None, None, 0) == -1
    assert amd.klt_hip_affine_state_put(None, buf, st, 1, C.byref(pa), C.byref(ps)) == -1
    assert pa.value is None and ps.value is None
    assert amd.klt_hip_affine_state_get(None, buf, st, 1) == -1
    for bad in (dict(mode=3), dict(mode=-1), dict(window=4), dict(window=1)):
        t = TrackingContextRec()
        affine_setup(**{"mode": 2, **bad})(t)
        assert amd.klt_hip_set_frames_affine(None, C.byref(AffineDesc.from_tc(t)), buf, st) == -1
