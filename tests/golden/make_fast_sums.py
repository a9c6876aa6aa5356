#!/usr/bin/env python3
"""The bound KLT_HIP_FAST is held to, measured on the CPU (tests/sum_scenes.py),
written to tests/golden/fast_sums_160x120.json.  Per configuration:

  scene, npx, ppl   the scene, the window's pixels, pixels per lane of the generic tracker's instance
  conditions        tracked compared cells and first-loss statuses of the SEQ table
  B                 4 x the largest p99 of d among the float orders below, at least 4 (ulps of a coordinate)
  orders            per float order run through the whole sequence and replayed one frame at a time against
                    the float64 statement: compared and tracked cells, status mismatches, p50 / p99 / max
                    of d, the cells that disagree at B and their share
  mutants           "<mutant>/<group of sums>": the share of disagreeing cells of that mistake

The section "gpu" is a record of the device's figures (tests/test_gpu_fast_sums.py
writes them per case where it runs); this script keeps it as it finds it.
Runs on the oracle alone (tests/native/build/libsums_oracle.so):

  python tests/golden/make_fast_sums.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import sum_scenes as ss  # noqa: E402


def main():
    old = json.loads(ss.FIXTURE.read_text()) if ss.FIXTURE.exists() else {}
    out = {"frames": "motion_scenes.scene, 160x120x14, the placed list of 251 features",
           "max_share": ss.MAX_SHARE, "max_order_share": ss.MAX_ORDER_SHARE,
           "configs": {}, "gpu": old.get("gpu", {})}
    for name in ss.CONFIGS:
        m = ss.measure(name)
        ss.check_conditions(name, m["conditions"])
        out["configs"][name] = m
        worst = max(m["orders"].values(), key=lambda f: f["share"])
        print(f"{name}: scene {m['scene']}, tracked {m['conditions']['tracked']}, B {m['B']}, "
              f"worst order share {worst['share']:.5f}, p99 {max(f['p99'] for f in m['orders'].values())}, "
              f"max d {max(f['max'] for f in m['orders'].values())}")
    ss.FIXTURE.write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {ss.FIXTURE} ({ss.FIXTURE.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
