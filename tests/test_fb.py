"""Forward-backward (FB) consistency check: the expected values and the host
side (no GPU needed).

The expected values are a composition of two plain KLTTrackFeatures steps
(include/klt_hip.h, klt_hip_set_fb): forward img1 -> img2 on a sequential
context, then the same call with the images exchanged on a copy of the result
and a second, NON-sequential context (the sequential one's kept pyramid is not
disturbed), then the verdict in float32 -- dx = xb - x0, dy = yb - y0,
e = dx*dx + dy*dy, five operations each rounded, rejected when the backward
step lost the feature or e > max_dist*max_dist.  `fb_compose` runs it on the
clean-room oracle (OracleStepper) or on any klt.h library (KltStepper: the
reference build for tests/golden/make_fb.py and the fixture test below).

tests/test_gpu_fb.py imports the composition from here.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import kltabi
from kltabi import GOLDEN, OracleParams, OracleTracker, arrays_to_fl, fl_to_arrays, u8ptr

FB_REJECTED = -6
FB_FIXTURE = GOLDEN / "fb_config1.json"


def fb_verdict(x0, y0, x, y, v, xb, yb, vb, max_dist):
    """The verdict on a forward result (x, y, v: changed in place) given the
    backward one; returns e per feature (-1 where there is no distance)."""
    t2 = np.float32(max_dist) * np.float32(max_dist)
    live = v >= 0
    dx = (xb - x0).astype(np.float32)
    dy = (yb - y0).astype(np.float32)
    e = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
    have = live & (vb >= 0)
    rej = live & ((vb < 0) | (e > t2))
    x[rej] = -1.0
    y[rej] = -1.0
    v[rej] = FB_REJECTED
    return np.where(have, e, np.float32(-1.0)).astype(np.float32)


class OracleStepper:
    """select / forward / backward / replace on the clean-room oracle."""

    def __init__(self, lib, params: OracleParams | None = None):
        if params is None:
            params = OracleParams()
            lib.orc_default_params(C.byref(params))
        pf, pb = OracleParams(), OracleParams()
        C.memmove(C.byref(pf), C.byref(params), C.sizeof(params))
        C.memmove(C.byref(pb), C.byref(params), C.sizeof(params))
        pf.sequentialMode, pb.sequentialMode = 1, 0
        self.f, self.b = OracleTracker(lib, pf), OracleTracker(lib, pb)

    def select(self, img, n):
        return self.f.select(img, n)

    def forward(self, a, b, x, y, v):
        self.f.track(a, b, x, y, v)

    def backward(self, a, b, x, y, v):
        self.b.track(a, b, x, y, v)

    def replace(self, img, x, y, v):
        self.f.replace(img, x, y, v)

    def close(self):
        self.f.close()
        self.b.close()


class KltStepper:
    """The same four steps on a klt.h library (two tracking contexts)."""

    def __init__(self, lib, n, setup=None):
        self.lib = lib
        self.tf, self.tb = lib.KLTCreateTrackingContext(), lib.KLTCreateTrackingContext()
        for tc, seq in ((self.tf, 1), (self.tb, 0)):
            if setup:
                setup(tc.contents)
            tc.contents.sequentialMode = seq
        self.fl = lib.KLTCreateFeatureList(n)

    def _run(self, tc, a, b, x, y, v):
        h, w = a.shape
        arrays_to_fl(self.fl, x, y, v)
        self.lib.KLTTrackFeatures(tc, u8ptr(np.ascontiguousarray(a)), u8ptr(np.ascontiguousarray(b)), w, h, self.fl)
        x[:], y[:], v[:] = fl_to_arrays(self.fl)

    def select(self, img, n):
        h, w = img.shape
        self.lib.KLTSelectGoodFeatures(self.tf, u8ptr(np.ascontiguousarray(img)), w, h, self.fl)
        return fl_to_arrays(self.fl)

    def forward(self, a, b, x, y, v):
        self._run(self.tf, a, b, x, y, v)

    def backward(self, a, b, x, y, v):
        self._run(self.tb, a, b, x, y, v)

    def replace(self, img, x, y, v):
        h, w = img.shape
        arrays_to_fl(self.fl, x, y, v)
        self.lib.KLTReplaceLostFeatures(self.tf, u8ptr(np.ascontiguousarray(img)), w, h, self.fl)
        x[:], y[:], v[:] = fl_to_arrays(self.fl)

    def close(self):
        self.lib.KLTFreeFeatureList(self.fl)
        self.lib.KLTFreeTrackingContext(self.tf)
        self.lib.KLTFreeTrackingContext(self.tb)


def fb_compose(st, frames, n, nframes, max_dist, first=None, replace=False, stats=None, start=None):
    """KLTRunner.harness's loop with the FB step after every track: X, Y, V
    ([n, nframes], column i-1 = the list after tracking frames[i], column 0
    overwritten like the harness does, the last never written) and E
    ([nframes-1, n], row i-1 = frame i's squared return distances).  stats (a
    dict): "rejected" receives the number of verdicts that rejected a feature
    (with replacement the table no longer shows them).  start: the list to
    track instead of a selection on the first image."""
    img1 = np.ascontiguousarray(frames[1] if first is None else first)
    X = np.zeros((n, nframes), np.float32)
    Y = np.zeros((n, nframes), np.float32)
    V = np.zeros((n, nframes), np.int32)
    E = np.full((nframes - 1, n), -1.0, np.float32)
    x, y, v = st.select(img1, n) if start is None else tuple(a.copy() for a in start)
    X[:, 0], Y[:, 0], V[:, 0] = x, y, v
    nrej = 0
    for i in range(1, nframes):
        img2 = np.ascontiguousarray(frames[i])
        x0, y0 = x.copy(), y.copy()
        st.forward(img1, img2, x, y, v)
        xb, yb, vb = x.copy(), y.copy(), v.copy()
        st.backward(img2, img1, xb, yb, vb)
        before = v == FB_REJECTED
        E[i - 1] = fb_verdict(x0, y0, x, y, v, xb, yb, vb, max_dist)
        nrej += int(((v == FB_REJECTED) & ~before).sum())
        if replace:
            st.replace(img2, x, y, v)
        X[:, i - 1], Y[:, i - 1], V[:, i - 1] = x, y, v
        img1 = img2
    st.close()
    if stats is not None:
        stats["rejected"] = nrej
    return X, Y, V, E


def fb_counts(V):
    """(features rejected by the check, features live) in the last written
    column: without replacement a rejected feature stays rejected"""
    return int((V[:, -2] == FB_REJECTED).sum()), int((V[:, -2] >= 0).sum())


def assert_splits(V):
    """A threshold meant to split does: at least 3 rejected, at least half kept."""
    rejected, live = fb_counts(V)
    assert rejected >= 3 and 2 * live >= V.shape[0], (rejected, live)


def load_fb_fixture():
    d = json.loads(FB_FIXTURE.read_text())
    hexf = lambda rows: np.array([[int(s, 16) for s in r] for r in rows], np.uint32).view(np.float32)  # noqa: E731
    X, Y, E = hexf(d["x"]), hexf(d["y"]), hexf(d["e"])
    return d, X, Y, np.array(d["val"], np.int32), E


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_constants():
    import kltamd.abi as abi
    import kltamd.device as dev
    assert abi.KLT_AMD_FB_REJECTED == -6 == dev.FB_REJECTED == FB_REJECTED
    assert abi.KLT_AMD_FB_REJECTED not in (abi.KLT_TRACKED, abi.KLT_NOT_FOUND, abi.KLT_SMALL_DET,
                                           abi.KLT_MAX_ITERATIONS, abi.KLT_OOB, abi.KLT_LARGE_RESIDUE)
    hdr = (kltabi.ROOT / "include" / "klt_amd.h").read_text()
    assert "#define KLT_AMD_FB_REJECTED -6" in hdr
    assert "KLT_AMD_FB_REJECTED" not in (kltabi.ROOT / "include" / "klt.h").read_text()
    for name in ("klt_hip_set_fb", "klt_hip_get_fb", "klt_hip_set_fb_table", "klt_amd_set_fb_check"):
        assert name in dev.DEVICE_PROTOS


def test_set_fb_check_arguments(amd, capfd):
    """Bad thresholds are refused with a warning and leave the context usable;
    the call needs no device."""
    tc = amd.KLTCreateTrackingContext()
    for ok in (0.0, 0.05, 1.0, 3.0e38):
        assert amd.klt_amd_set_fb_check(tc, 1, ok) == 0
    assert amd.klt_amd_set_fb_check(tc, 0, 0.5) == 0
    capfd.readouterr()
    for bad in (-0.001, -1.0, float("nan"), float("inf"), float("-inf")):
        assert amd.klt_amd_set_fb_check(tc, 1, bad) == -1, bad
        assert "klt_amd_set_fb_check" in capfd.readouterr().err
    amd.KLTFreeTrackingContext(tc)


@pytest.mark.parametrize("fmt", [None, b"%5.1f"])
def test_rejected_code_round_trips_through_tables(amd, tmp_path, fmt):
    """A table holding -6 cells writes and reads back, binary and text."""
    nfeat, nframes = 7, 4
    ft = amd.KLTCreateFeatureTable(nframes, nfeat)
    want = np.zeros((nfeat, nframes), np.int32)
    for j in range(nfeat):
        for i in range(nframes):
            f = ft.contents.feature[j][i].contents
            lost = (i + j) % 3 == 0 and i > 0
            f.x, f.y = (-1.0, -1.0) if lost else (10.5 + j, 20.25 + i)
            f.val = FB_REJECTED if lost else 0
            want[j, i] = f.val
    assert (want == FB_REJECTED).sum() >= 3
    path = str(tmp_path / ("t.txt" if fmt else "t.ft")).encode()
    amd.KLTWriteFeatureTable(ft, path, fmt)
    back = amd.KLTReadFeatureTable(None, path)
    assert back and back.contents.nFrames == nframes and back.contents.nFeatures == nfeat
    for j in range(nfeat):
        for i in range(nframes):
            a, b = ft.contents.feature[j][i].contents, back.contents.feature[j][i].contents
            assert b.val == want[j, i]
            if fmt is None:
                assert (a.x, a.y) == (b.x, b.y)
            else:
                assert abs(a.x - b.x) <= 0.051 and abs(a.y - b.y) <= 0.051
    fl = amd.KLTCreateFeatureList(nfeat)
    amd.KLTExtractFeatureList(fl, back, 1)
    assert amd.KLTCountRemainingFeatures(fl) == int((want[:, 1] >= 0).sum())
    amd.KLTFreeFeatureList(fl)
    amd.KLTFreeFeatureTable(back)
    amd.KLTFreeFeatureTable(ft)


def test_fixture_shape():
    d, X, Y, V, E = load_fb_fixture()
    assert (d["dataset"], d["features"], d["frames"], d["max_dist"]) == ("images_provided", 100, 10, 0.05)
    assert X.shape == Y.shape == V.shape == (100, 10) and E.shape == (9, 100)
    assert fb_counts(V) == (23, 59)
    assert_splits(V)


def test_oracle_composition_equals_fixture(oracle, frames):
    d, X, Y, V, E = load_fb_fixture()
    OX, OY, OV, OE = fb_compose(OracleStepper(oracle), frames, 100, 10, d["max_dist"], first=frames[0])
    assert np.array_equal(OV, V)
    assert np.array_equal(bits(OX), bits(X)) and np.array_equal(bits(OY), bits(Y))
    assert np.array_equal(bits(OE), bits(E))


def test_reference_composition_reproduces_fixture(ref, frames):
    """Where oracle/_ref is built: the fixture is what the reference computes."""
    d, X, Y, V, E = load_fb_fixture()
    ref.KLTSetVerbosity(0)
    RX, RY, RV, RE = fb_compose(KltStepper(ref, 100), frames, 100, 10, d["max_dist"], first=frames[0])
    assert np.array_equal(RV, V)
    assert np.array_equal(bits(RX), bits(X)) and np.array_equal(bits(RY), bits(Y))
    assert np.array_equal(bits(RE), bits(E))


@pytest.mark.parametrize("max_dist,rejected,live", [(0.05, 23, 59), (0.02, 81, 8), (1.0, 0, 80)])
def test_oracle_composition_counts(oracle, frames, max_dist, rejected, live):
    """Both outcomes occur on images_provided, and no e is within 4 ulp of the
    threshold, so no verdict hangs on a tie."""
    X, Y, V, E = fb_compose(OracleStepper(oracle), frames, 100, 10, max_dist, first=frames[0])
    got = fb_counts(V)
    assert got == (rejected, live)
    t2 = np.float32(max_dist) * np.float32(max_dist)
    have = E >= 0
    assert (np.abs(bits(E)[have].astype(np.int64) - int(t2.view(np.int32))) > 4).all()
