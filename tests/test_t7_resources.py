"""Register budget of the two-level lazy-gradient trackers, from the code
object's metadata (tools/t7_resources.py builds the device assembly of
csrc/track7.hip with the Makefile's flags).  No GPU; skipped without hipcc.

The four instances -- k_track7<false, true, 2, {false, true}, true> and
k_track7_hook<2, {false, true}> -- must hold five waves per SIMD: at most 96
VGPRs, no vector spill, no scratch.  Their scalar spills were 48, 42, 55 and 52
lanes of the spill register, written before the frame loop and read back
about 110 times inside it; they are 6, 4, 14 and 13 now (a mask or two and
one loop-carried count), and the bound here is a quarter of the spill
register's 64 lanes, so that a return to the old state fails.  Only the
metadata's counts are read; instructions are not scanned.
"""
from __future__ import annotations

import importlib.util
import os
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TARGETS = ("k_track7<false, true, 2, false, true>", "k_track7<false, true, 2, true, true>",
           "k_track7_hook<2, false>", "k_track7_hook<2, true>")
MAX_SCALAR_SPILLS = 16


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists(
        "/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not _hipcc():
        pytest.skip("hipcc not found")
    spec = importlib.util.spec_from_file_location("t7_resources", ROOT / "tools" / "t7_resources.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["t7_resources"] = mod
    spec.loader.exec_module(mod)
    asm = tmp_path_factory.mktemp("t7") / "track7.s"
    mod.assemble(str(ROOT / "klt-feature-tracker-acceleration-gpus_amd" / "csrc" / "track7.hip"), str(asm))
    meta = mod.metadata(asm.read_text().splitlines())
    names = mod.demangle(list(meta))
    return {names[k]: v for k, v in meta.items()}


@pytest.mark.parametrize("name", TARGETS)
def test_two_level_lazy_instances(kernels, name):
    m = kernels[name]
    print(name, m)
    assert m["vgpr_count"] <= 96 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["sgpr_spill_count"] <= MAX_SCALAR_SPILLS, m
    assert m["group_segment_fixed_size"] <= 15296 + 64, m


def test_every_tracker_is_listed(kernels):
    """All nineteen k_track7* instances are in the code object and none uses
    scratch: the full-record, band, fb and multi ones as well."""
    assert len(kernels) == 19 and all(m["private_segment_fixed_size"] == 0 for m in kernels.values()), kernels
