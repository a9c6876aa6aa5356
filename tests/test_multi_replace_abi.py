"""Replacement inside the multi-sequence call at the library boundary: the new
symbols through the package's bindings, their signatures, and the argument
checks that touch no GPU (klt_hip_track_frames_multi_replace,
klt_hip_min_eigen_records, KLTTrackSequencesReplace)."""
from __future__ import annotations

import ctypes as C
import subprocess
import sys

from kltabi import ROOT

NEW_DEVICE = ("klt_hip_track_frames_multi_replace", "klt_hip_min_eigen_records")


def test_symbols_are_bound(amd):
    from kltamd import abi, device
    for name in NEW_DEVICE:
        res, args = device.DEVICE_PROTOS[name]
        fn = getattr(amd, name)
        assert fn.restype is res is C.c_int and list(fn.argtypes) == list(args), name
    # ctx, pdesc, tdesc, rep, count0 | the 15 of klt_hip_track_frames_multi | changed, runs, filled
    multi = device.DEVICE_PROTOS["klt_hip_track_frames_multi"][1]
    args = device.DEVICE_PROTOS["klt_hip_track_frames_multi_replace"][1]
    assert len(args) == 23 and len(multi) == 18
    assert args[:3] == multi[:3] and args[5:20] == multi[3:]
    assert args[3]._type_ is device.ReplaceDesc and args[4] is C.c_long
    assert len(device.DEVICE_PROTOS["klt_hip_min_eigen_records"][1]) == 9
    res, args = abi.AMD_KLT_PROTOS["KLTTrackSequencesReplace"]
    fn = amd.KLTTrackSequencesReplace
    assert fn.restype is res is None and list(fn.argtypes) == list(args) and len(args) == 10
    assert args[:9] == abi.AMD_KLT_PROTOS["KLTTrackSequences"][1] and args[9] is C.c_int


def test_null_context_is_an_error_not_a_crash(amd):
    from kltamd.device import PyrDesc, ReplaceDesc, SelectDesc, TrackDesc
    pd, td = PyrDesc(), TrackDesc()
    sd = SelectDesc(7, 7, 24, 24, 0)
    rd = ReplaceDesc(sd, 10, 1, 3)
    n_seq = (C.c_int * 1)(0)
    which = (C.c_int * 1)(0)
    assert amd.klt_hip_track_frames_multi_replace(None, C.byref(pd), C.byref(td), C.byref(rd), 0, None, 0, 0, 0, 1, 0,
                                                  1, n_seq, None, None, None, None, None, None, 0, None, None,
                                                  None) == -1
    assert amd.klt_hip_min_eigen_records(None, None, 0, which, 1, 8, 8, C.byref(sd), None) == -1


def test_every_below_one_is_a_klt_error():
    """KLTTrackSequencesReplace checks `every` before it touches a device: the
    child ends on that error where no device exists (there, asking for a device
    context first would be another error)."""
    code = ("import sys; sys.path.insert(0, %r); import kltamd, numpy as np, ctypes as C;"
            "from kltamd.abi import U8P, FL;"
            "lib = kltamd.load(); lib.KLTSetVerbosity(0);"
            "tc = lib.KLTCreateTrackingContext(); fl = lib.KLTCreateFeatureList(5);"
            "a = np.zeros((64, 64), np.uint8); p = a.ctypes.data_as(U8P);"
            "arr = (U8P * 2)(p, p); frames = (C.POINTER(U8P) * 1)(C.cast(arr, C.POINTER(U8P)));"
            "fls = (FL * 1)(fl);"
            "lib.KLTTrackSequencesReplace(tc, frames, 1, 2, 64, 64, fls, None, 0, 0); print('returned')") % str(ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 1 and "KLT Error" in r.stderr and "every=0" in r.stderr, (r.returncode, r.stderr[-500:])
    assert "KLTTrackSequencesReplace" in r.stderr
    assert "returned" not in r.stdout
