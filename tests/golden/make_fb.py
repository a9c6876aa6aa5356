#!/usr/bin/env python3
"""Regenerate tests/golden/fb_config1.json from the REFERENCE itself.

The forward-backward check is two plain KLTTrackFeatures calls and a float32
compare (tests/test_fb.py: fb_compose), so the reference library computes its
expected values: images_provided, 100 features selected on image 0 and tracked
through images 1..9, a sequential
forward context, a non-sequential backward one, max_dist 0.05.  Needs
oracle/_ref/ (`make -C oracle ref`), like make_golden.py.  Data only: per
frame x, y and e as hex bit patterns of the floats, and val.

  python tests/golden/make_fb.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from kltabi import REF_LIB, bind_klt, load_dataset  # noqa: E402
from test_fb import FB_FIXTURE, KltStepper, fb_compose, fb_counts  # noqa: E402

N, FRAMES, MAX_DIST = 100, 10, 0.05


def hexrows(a: np.ndarray) -> list[list[str]]:
    return [[f"{w:08x}" for w in row] for row in np.ascontiguousarray(a, np.float32).view(np.uint32)]


def main() -> None:
    if not REF_LIB.exists():
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` (needs /root/reference)")
    ref = bind_klt(REF_LIB)
    ref.KLTSetVerbosity(0)
    frames = load_dataset()
    X, Y, V, E = fb_compose(KltStepper(ref, N), frames, N, FRAMES, MAX_DIST, first=frames[0])
    rejected, live = fb_counts(V)
    out = {
        "dataset": "images_provided", "features": N, "frames": FRAMES, "max_dist": MAX_DIST,
        "layout": "features selected on image 0; x, y, val: [feature][column], column i-1 = the list after "
                  "tracking image i (the last column is never written); e: [i-1][feature], -1 = no distance; "
                  "floats as hex bit patterns",
        "rejected": rejected, "live_at_end": live,
        "x": hexrows(X), "y": hexrows(Y), "val": V.tolist(), "e": hexrows(E),
    }
    FB_FIXTURE.write_text(json.dumps(out, separators=(",", ":")) + "\n")
    print(f"wrote {FB_FIXTURE}: {rejected} rejected, {live} live at the end")


if __name__ == "__main__":
    main()
