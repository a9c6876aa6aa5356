"""Register and LDS budget of the level-0 pyramid kernels, from the code
object's metadata (tools/t7_resources.py builds the device assembly of
csrc/pyramid.hip with the Makefile's flags).  No GPU; skipped without hipcc.

k_pyr_l0s, the one-wave strip kernel, must fit eight waves per SIMD and any
wave slot a tracker wave frees: at most 64 VGPRs, no scratch, at most 4 KB of
LDS.  The tile instances keep the figures of DESIGN section 4's resource table
(58 VGPRs, no scratch; 33 440, 25 152 and 48 192 bytes of LDS): the default
path changed, the tile kernels did not.  Only the metadata's counts are read;
instructions are not scanned.
"""
from __future__ import annotations

import importlib.util
import os
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
# instance: (VGPRs, LDS bytes) of DESIGN's table
TILES = {"k_pyr_l0<true, 32, false>": (58, 33440), "k_pyr_l0<false, 32, true>": (58, 25152),
         "k_pyr_l0<false, 64, true>": (58, 48192)}


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
    asm = tmp_path_factory.mktemp("l0s") / "pyramid.s"
    mod.assemble(str(ROOT / "klt-feature-tracker-acceleration-gpus_amd" / "csrc" / "pyramid.hip"), str(asm))
    meta = mod.metadata(asm.read_text().splitlines())
    names = mod.demangle(list(meta))
    return {names[k]: v for k, v in meta.items()}


def test_strip_kernel(kernels):
    strips = {n: m for n, m in kernels.items() if n.startswith("k_pyr_l0s<")}
    assert len(strips) == 1, list(kernels)
    for name, m in strips.items():
        print(name, m)
        assert m["vgpr_count"] <= 64 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
        assert m["group_segment_fixed_size"] <= 4096, m


@pytest.mark.parametrize("name", sorted(TILES))
def test_tile_instances_unchanged(kernels, name):
    m = kernels[name]
    print(name, m)
    vgprs, lds = TILES[name]
    assert m["vgpr_count"] == vgprs and m["private_segment_fixed_size"] == 0, m
    assert m["group_segment_fixed_size"] == lds, m
