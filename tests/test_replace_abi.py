"""The replacement setting's ABI without a device: the new symbols through the
package's bindings, klt_hip_replace_desc's layout against the header, and the
argument checks that touch no GPU."""
from __future__ import annotations

import ctypes as C
import subprocess
import sys
import tempfile
from pathlib import Path

from kltabi import ROOT

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "klt_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(klt_hip_replace_desc), offsetof(klt_hip_replace_desc, sel),
         offsetof(klt_hip_replace_desc, mindist), offsetof(klt_hip_replace_desc, min_eigenvalue),
         offsetof(klt_hip_replace_desc, every));
  return 0;
}
"""


def test_replace_desc_layout_equals_the_header():
    from kltamd.device import ReplaceDesc
    with tempfile.TemporaryDirectory() as d:
        src, exe = Path(d) / "probe.c", Path(d) / "probe"
        src.write_text(PROBE)
        subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(ReplaceDesc), ReplaceDesc.sel.offset, ReplaceDesc.mindist.offset,
                   ReplaceDesc.min_eigenvalue.offset, ReplaceDesc.every.offset] == [32, 0, 20, 24, 28]


def test_symbols_are_bound(amd):
    from kltamd.abi import AMD_KLT_PROTOS
    from kltamd.device import DEVICE_PROTOS
    assert "KLTTrackSequenceReplace" in AMD_KLT_PROTOS
    assert len(amd.KLTTrackSequenceReplace.argtypes) == 9
    for name in ("klt_hip_set_frames_replace", "klt_hip_get_frames_replace", "klt_hip_frames_replace_changed",
                 "klt_hip_min_eigen_plane", "klt_hip_eigen_kernel"):
        assert name in DEVICE_PROTOS and getattr(amd, name).argtypes is not None


def test_from_tc_maxes_the_borders(amd):
    from kltamd.device import ReplaceDesc
    tc = amd.KLTCreateTrackingContext()
    t = tc.contents
    t.borderx, t.bordery, t.nSkippedPixels, t.mindist, t.min_eigenvalue = 1, 30, 1, 12, 5
    rd = ReplaceDesc.from_tc(t, 4)
    assert (rd.sel.window_width, rd.sel.window_height, rd.sel.borderx, rd.sel.bordery, rd.sel.nSkippedPixels) == \
           (7, 7, 3, 30, 1)
    assert (rd.mindist, rd.min_eigenvalue, rd.every) == (12, 5, 4)
    amd.KLTFreeTrackingContext(tc)


def test_null_context_is_refused(amd):
    from kltamd.device import ReplaceDesc, SelectDesc
    rd = ReplaceDesc(SelectDesc(7, 7, 24, 24, 0), 10, 1, 1)
    assert amd.klt_hip_set_frames_replace(None, C.byref(rd)) == -1
    assert amd.klt_hip_get_frames_replace(None, None, None, None, None) == -1
    assert amd.klt_hip_frames_replace_changed(None, None, 0) == -1
    assert amd.klt_hip_min_eigen_plane(None, None, 8, 8, None, None) == -1
    assert amd.klt_hip_eigen_kernel(None) == b""


def test_every_below_one_is_a_klt_error():
    """KLTTrackSequenceReplace checks `every` before it touches a device."""
    code = ("import sys; sys.path.insert(0, %r); import kltamd, numpy as np, ctypes as C;"
            "lib = kltamd.load(); lib.KLTSetVerbosity(0);"
            "tc = lib.KLTCreateTrackingContext(); fl = lib.KLTCreateFeatureList(5);"
            "a = np.zeros((64, 64), np.uint8); p = a.ctypes.data_as(kltamd.abi.U8P);"
            "arr = (kltamd.abi.U8P * 2)(p, p);"
            "lib.KLTTrackSequenceReplace(tc, arr, 2, 64, 64, fl, None, 0, 0); print('returned')") % str(ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 1 and "KLT Error" in r.stderr and "every=0" in r.stderr, (r.returncode, r.stderr[-500:])
    assert "returned" not in r.stdout
