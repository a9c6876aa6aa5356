"""The multi-sequence calls at the library boundary: exported symbols and
ctypes signatures (klt_hip_track_frames_multi, klt_hip_multi_covers,
KLTTrackSequences).  Runs without a GPU."""
from __future__ import annotations

import ctypes as C

NEW_DEVICE = ("klt_hip_track_frames_multi", "klt_hip_multi_covers")
NEW_KLT = ("KLTTrackSequences",)


def test_symbols_are_exported(amd):
    for name in NEW_DEVICE + NEW_KLT:
        assert hasattr(amd, name), name


def test_signatures_bind(amd):
    from kltamd import abi, device
    for name in NEW_DEVICE:
        res, args = device.DEVICE_PROTOS[name]
        fn = getattr(amd, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # frames, pitch, stride, seq_stride, nseq, nframes, chunk, n_seq, x, y, val, tab_x, tab_y, tab_val, tab_stride
    res, args = device.DEVICE_PROTOS["klt_hip_track_frames_multi"]
    assert res is C.c_int and len(args) == 18
    assert args[4:10] == [C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int] and args[-1] is C.c_long
    res, args = abi.AMD_KLT_PROTOS["KLTTrackSequences"]
    fn = amd.KLTTrackSequences
    assert fn.restype is res is None and list(fn.argtypes) == list(args) and len(args) == 9
    assert device.MAX_SEQUENCES == 64


def test_null_context_is_an_error_not_a_crash(amd):
    """Both device calls check their arguments before touching a device."""
    from kltamd.device import PyrDesc, TrackDesc
    pd, td = PyrDesc(), TrackDesc()
    n_seq = (C.c_int * 1)(0)
    assert amd.klt_hip_multi_covers(None, C.byref(pd), C.byref(td)) == -1
    assert amd.klt_hip_track_frames_multi(None, C.byref(pd), C.byref(td), None, 0, 0, 0, 1, 0, 1, n_seq, None, None,
                                          None, None, None, None, 0) == -1
