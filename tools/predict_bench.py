#!/usr/bin/env python3
"""What the motion prior (klt_hip_set_predict) costs on the device-resident
batched path, at bench.py's headline shape: 1080p, 5000 features selected on
frame 0, synthetic seed 1080, klt_hip_track_frames in 64-frame chunks.

Setting off and setting on alternate, `--rounds` times in one process, each
from the same selection state (and a zero prior) over the same frames:
frames/s over a host clock around the call and a device synchronise, and -- in
a replay of its own with events on -- the tracker's microseconds per frame from
klt_hip_get_timing.  With the setting on the tracker reads full level-0 records
(no lazy gradients), takes the residue pass in place and carries no corners, so
it is expected to be slower; the synthetic frames move by less than a pixel, so
the prior saves nothing here and the two runs' live counts are reported only
to show that.  bench.py and its headline are not involved.

Prints one JSON line.  Needs a GPU; there is no fallback.

  python tools/predict_bench.py [--frames 256] [--rounds 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=256, help="tracked frames per run")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("--rounds: at least 3")

    import kltamd
    from kltamd.device import D2H, H2D, PyrDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("predict_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    W, H, NF, T = args.width, args.height, args.features, args.frames
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = lib.klt_amd_device_context(tc)
    ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731

    nfr = T + 1
    dfr = lib.klt_hip_malloc(ctx, nfr * W * H)
    ck(lib.klt_hip_synth_frames(ctx, args.seed, 0, nfr, W, H, dfr, W, W * H), "synth")
    f0 = np.empty((H, W), np.uint8)
    ck(lib.klt_hip_memcpy(ctx, f0.ctypes.data, dfr, f0.nbytes, D2H), "frame 0")
    fl = lib.KLTCreateFeatureList(NF)
    lib.KLTSelectGoodFeatures(tc, f0.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, fl)
    x0 = np.array([fl.contents.feature[k].contents.x for k in range(NF)], np.float32)
    y0 = np.array([fl.contents.feature[k].contents.y for k in range(NF)], np.float32)
    v0 = np.array([fl.contents.feature[k].contents.val for k in range(NF)], np.int32)
    z0 = np.zeros(NF, np.float32)
    lib.KLTFreeFeatureList(fl)
    dx, dy, dv, dvx, dvy = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(5))
    tx, ty, tv = (lib.klt_hip_malloc(ctx, 4 * NF * T) for _ in range(3))
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))

    def reset():
        for d, a in ((dx, x0), (dy, y0), (dv, v0), (dvx, z0), (dvy, z0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
        ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
        ck(lib.klt_hip_sync(ctx), "sync")

    def batched(on, timing=False):
        """One run over the T frames; returns seconds (host clock, synchronised)."""
        ck(lib.klt_hip_set_predict(ctx, 1 if on else 0, dvx if on else None, dvy if on else None), "set_predict")
        reset()
        ck(lib.klt_hip_set_timing(ctx, 1 if timing else 0), "timing")
        t0 = time.perf_counter()
        rc = lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + W * H, W, W * H, T, args.chunk, dx, dy, dv,
                                      NF, tx, ty, tv, NF)
        ck(lib.klt_hip_sync(ctx), "sync")
        dt = time.perf_counter() - t0
        ck(rc, "track_frames")
        return dt

    def live():
        V = np.empty((T, NF), np.int32)
        ck(lib.klt_hip_memcpy(ctx, V.ctypes.data, tv, V.nbytes, D2H), "d2h")
        return int((V[-1] >= 0).sum())

    # warm-up: both kernels' code objects, the banks, the sustained clock
    w0 = time.perf_counter()
    while time.perf_counter() - w0 < 0.5:
        batched(False)
        batched(True)
    rate = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            rate[on].append(T / batched(on))
    live_on = live()  # the last run had the setting on
    kernel_on = lib.klt_hip_track_kernel(ctx).decode()

    # the tracker's own time, events on (a run of its own: events serialise the launches' timing)
    us = {}
    tm = Timing()
    for on in (False, True):
        vals = []
        for _ in range(args.rounds):
            batched(on, timing=True)
            ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
            vals.append(1e3 * tm.ms_track / max(1, tm.frames_track))
        us[on] = vals
    ck(lib.klt_hip_set_timing(ctx, 0), "timing off")
    batched(False)
    live_off = live()
    kernel_off = lib.klt_hip_track_kernel(ctx).decode()

    med = statistics.median
    out = {
        "tool": "predict_bench", "width": W, "height": H, "features": NF, "seed": args.seed, "frames": T,
        "chunk": args.chunk, "chunk_used": lib.klt_hip_frames_chunk(ctx), "rounds": args.rounds,
        "fps_off": [round(r, 1) for r in rate[False]], "fps_on": [round(r, 1) for r in rate[True]],
        "fps_off_median": round(med(rate[False]), 1), "fps_on_median": round(med(rate[True]), 1),
        "fps_on_over_off": round(med(rate[True]) / med(rate[False]), 4),
        "tracker_us_per_frame_off": [round(u, 3) for u in us[False]],
        "tracker_us_per_frame_on": [round(u, 3) for u in us[True]],
        "tracker_us_on_over_off": round(med(us[True]) / med(us[False]), 3),
        "kernel_off": kernel_off, "kernel_on": kernel_on,
        "live_at_end_off": live_off, "live_at_end_on": live_on,
    }
    ck(lib.klt_hip_set_predict(ctx, 0, None, None), "set_predict off")
    for d in (dfr, dx, dy, dv, dvx, dvy, tx, ty, tv):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
