#!/usr/bin/env python3
"""The reference's tables on the rotating scenes of tests/motion_scenes.py
(tests/test_motion_host.py, tests/test_gpu_motion.py), written to
tests/golden/motion_160x120.npz:

  sha_<seed>, sha_shard_<seed>   sha256 of the stacked frames (160x120x14, 320x240x11)
  placed_x / _y / _v             the placed list
  <config>_<seed>_X / _Y / _V    [13, 251]: KLTTrackFeatures per frame from the placed
                                 list, sequential mode, for the configurations
                                 default, maxit3, lighting, win9, one_level
  sel100_<seed>_x / _y / _v      KLTSelectGoodFeatures on frame 0, 100 asked
  harness100_<seed>_X / _Y / _V  [100, 14]: select, then track + KLTReplaceLostFeatures
                                 per frame (KLTRunner.harness, first = frame 0)

Tables only; the frames come from the generator.  The archive is written with
fixed member times, so the same tables give the same bytes.  Needs oracle/_ref
(built from the reference by __graft_entry__.build()).

  python tests/golden/make_motion.py
"""
from __future__ import annotations

import hashlib
import io
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from kltabi import GOLDEN, REF_LIB, KLTRunner, bind_klt, fl_to_arrays, u8ptr  # noqa: E402
import motion_scenes as ms  # noqa: E402


def frames_sha(frames) -> str:
    return hashlib.sha256(np.stack(frames).tobytes()).hexdigest()


def write_npz(path: Path, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def select(lib, frame, n):
    h, w = frame.shape
    tc = lib.KLTCreateTrackingContext()
    fl = lib.KLTCreateFeatureList(n)
    lib.KLTSelectGoodFeatures(tc, u8ptr(frame), w, h, fl)
    out = fl_to_arrays(fl)
    lib.KLTFreeFeatureList(fl)
    lib.KLTFreeTrackingContext(tc)
    return out


def main() -> None:
    if not REF_LIB.exists():
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` (needs the reference's sources)")
    ref = bind_klt(REF_LIB)
    ref.KLTSetVerbosity(0)
    out = {}
    start = ms.placed_list()
    out["placed_x"], out["placed_y"], out["placed_v"] = start
    for seed in ms.SCENES:
        frames = ms.scene(seed)
        out[f"sha_{seed}"] = np.array(frames_sha(frames))
        out[f"sha_shard_{seed}"] = np.array(frames_sha(ms.shard_scene(seed)))
        for name in ms.RECORDED:
            X, Y, V = ms.klt_table(ref, frames, start, ms.tc_setup(ref, name))
            out[f"{name}_{seed}_X"], out[f"{name}_{seed}_Y"], out[f"{name}_{seed}_V"] = X, Y, V
            print(f"{name} scene {seed}: {ms.status_counts(V)}")
        out[f"sel100_{seed}_x"], out[f"sel100_{seed}_y"], out[f"sel100_{seed}_v"] = select(ref, frames[0], 100)
        X, Y, V = KLTRunner(ref).harness(frames, 100, ms.NFRAMES, first=frames[0], replace=True)
        out[f"harness100_{seed}_X"], out[f"harness100_{seed}_Y"], out[f"harness100_{seed}_V"] = X, Y, V
    write_npz(ms.FIXTURE, out)
    man_path = GOLDEN / "manifest.json"
    man = json.loads(man_path.read_text())
    man[ms.FIXTURE.name] = hashlib.sha256(ms.FIXTURE.read_bytes()).hexdigest()
    man_path.write_text(json.dumps(man, indent=1, sort_keys=True) + "\n")
    print(f"wrote {ms.FIXTURE} ({ms.FIXTURE.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
