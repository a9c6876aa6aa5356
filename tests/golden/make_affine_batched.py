#!/usr/bin/env python3
"""Fixtures for the affine consistency check inside the batched tracker launch
(tests/test_affine_batched.py, tests/test_gpu_affine_batched.py): the
reference's own outputs, written by make_golden.write_affine's recipe -- X, Y,
V, AFF, HAS, CRC per frame -- for affine windows that cross, or stay below,
the 256-pixel chunk of the per-call kernel and the 64-lane wave:

  17x17 = 289 pixels   more than one 256-pixel chunk
  23x23 = 529 pixels   three of them
   5x5  =  25 pixels   less than one wave

Needs oracle/_ref (built from the reference by __graft_entry__.build()).

  python tests/golden/make_affine_batched.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from kltabi import GOLDEN, REF_LIB, affine_setup, bind_klt, run_affine  # noqa: E402
from make_golden import affine_inputs  # noqa: E402

# name, dataset, features, frames, replace, affine_setup arguments (AFFINE_CASES' layout)
BATCHED_CASES = [
    ("affine_batched_m2_w17_100x10", "images_provided", 100, 10, False,
     dict(mode=2, window=17, mdd=3.0, max_res=20.0)),
    ("affine_batched_m2_w23_100x10", "images_provided", 100, 10, False,
     dict(mode=2, window=23, mdd=3.0, max_res=20.0)),
    ("affine_batched_m1_w5_100x10", "images_provided", 100, 10, False, dict(mode=1, window=5)),
    ("affine_batched_m2_w5_100x10", "images_provided", 100, 10, False, dict(mode=2, window=5)),
    ("affine_batched_m0_li_w17_100x10", "images_provided", 100, 10, False, dict(mode=0, window=17, li=1)),
]


def main() -> None:
    if not REF_LIB.exists():
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` (needs the reference's sources)")
    ref = bind_klt(REF_LIB)
    ref.KLTSetVerbosity(0)
    for name, data, n, nf, replace, kw in BATCHED_CASES:
        X, Y, V, A, H, K = run_affine(ref, affine_inputs(data), n, nf, affine_setup(**kw), replace=replace)
        np.savez_compressed(GOLDEN / f"{name}.npz", X=X, Y=Y, V=V, AFF=A, HAS=H, CRC=K)
        held = H[-1] == 1
        lost = int(((H[:-1] == 1) & (H[1:] == 0)).any(axis=0).sum())
        off = float(np.abs(A[-1][held][:, 2:] - np.array([1, 0, 0, 1], np.float32)).max()) if held.any() else 0.0
        print(f"{name}: {int(held.sum())} windows held at the end, {lost} features lost a held window, "
              f"max |A - I| {off:.3f}")


if __name__ == "__main__":
    main()
