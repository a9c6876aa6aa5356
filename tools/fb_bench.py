#!/usr/bin/env python3
"""What the forward-backward check (klt_hip_set_fb) costs on the device-resident
batched path, at bench.py's headline shape: 1080p, 5000 features selected on
frame 0, synthetic seed 1080, klt_hip_track_frames in 64-frame chunks.

FB off and FB on alternate, `--rounds` times in one process, each from the same
selection state over the same frames: frames/s over a host clock around the
call and a device synchronise, and -- in a replay of its own with events on --
the tracker's microseconds per frame from klt_hip_get_timing.  For comparison,
what a caller could do without the fused kernels: per frame two klt_hip_track
calls on device arrays with the slots exchanged (the backward one on a copy of
the list), then the verdict on the host, which is also checked against the
fused result (bit patterns of x and y, val).

Prints one JSON line.  Needs a GPU; there is no fallback.

  python tools/fb_bench.py [--frames 256] [--rounds 3] [--max-dist 0.05]
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

FB_REJECTED = -6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=256, help="tracked frames per run")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-dist", type=float, default=0.05)
    ap.add_argument("--two-call-frames", type=int, default=64, help="frames of the two-call comparison")
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("--rounds: at least 3")

    import kltamd
    from kltamd.device import D2D, D2H, H2D, PyrDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("fb_bench: no HIP device visible")
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
    lib.KLTFreeFeatureList(fl)
    dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(3))
    tx, ty, tv, te = (lib.klt_hip_malloc(ctx, 4 * NF * T) for _ in range(4))
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))

    def reset():
        for d, a in ((dx, x0), (dy, y0), (dv, v0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
        ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
        ck(lib.klt_hip_sync(ctx), "sync")

    def batched(fb, timing=False):
        """One run over the T frames; returns seconds (host clock, synchronised)."""
        ck(lib.klt_hip_set_fb(ctx, 1 if fb else 0, args.max_dist), "set_fb")
        ck(lib.klt_hip_set_fb_table(ctx, te if fb else None, NF), "fb table")
        reset()
        ck(lib.klt_hip_set_timing(ctx, 1 if timing else 0), "timing")
        t0 = time.perf_counter()
        rc = lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + W * H, W, W * H, T, args.chunk, dx, dy, dv,
                                      NF, tx, ty, tv, NF)
        ck(lib.klt_hip_sync(ctx), "sync")
        dt = time.perf_counter() - t0
        ck(rc, "track_frames")
        return dt

    def table():
        X, Y, V = np.empty((T, NF), np.float32), np.empty((T, NF), np.float32), np.empty((T, NF), np.int32)
        for d, a in ((tx, X), (ty, Y), (tv, V)):
            ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return X, Y, V

    # warm-up: both kernels' code objects, the banks, the sustained clock
    w0 = time.perf_counter()
    while time.perf_counter() - w0 < 0.5:
        batched(False)
        batched(True)
    rate = {False: [], True: []}
    for _ in range(args.rounds):
        for fb in (False, True):
            rate[fb].append(T / batched(fb))
    X, Y, V = table()  # the last run had FB on
    kernel_fb = lib.klt_hip_track_kernel(ctx).decode()
    rej_cells = V == FB_REJECTED
    new_rej = rej_cells.copy()
    new_rej[1:] &= ~rej_cells[:-1]
    live_on = int((V[-1] >= 0).sum())

    # the tracker's own time, events on (a run of its own: events serialise the launches' timing)
    us = {}
    tm = Timing()
    for fb in (False, True):
        vals = []
        for _ in range(args.rounds):
            batched(fb, timing=True)
            ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
            vals.append(1e3 * tm.ms_track / max(1, tm.frames_track))
        us[fb] = vals
    ck(lib.klt_hip_set_timing(ctx, 0), "timing off")
    batched(False)
    live_off = int((table()[2][-1] >= 0).sum())
    kernel_off = lib.klt_hip_track_kernel(ctx).decode()

    # what is possible without the fused kernels: two klt_hip_track calls per
    # frame with the slots exchanged, and the verdict on the host
    TT = min(T, args.two_call_frames)
    bx, by, bv = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(3))
    ck(lib.klt_hip_set_fb(ctx, 0, 0.0), "fb off")
    ck(lib.klt_hip_set_fb_table(ctx, None, 0), "fb table off")
    t2 = np.float32(args.max_dist) * np.float32(args.max_dist)

    def two_call():
        for d, a in ((dx, x0), (dy, y0), (dv, v0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_build_pyramid(ctx, 0, C.byref(pd), dfr, W, 0), "build")
        ck(lib.klt_hip_sync(ctx), "sync")
        x, y, v = x0.copy(), y0.copy(), v0.copy()
        xb, yb, vb = np.empty_like(x), np.empty_like(y), np.empty_like(v)
        x1, y1, v1 = np.empty_like(x), np.empty_like(y), np.empty_like(v)
        cur = 0
        t0 = time.perf_counter()
        for t in range(1, TT + 1):
            nxt = 1 - cur
            ck(lib.klt_hip_build_pyramid(ctx, nxt, C.byref(pd), dfr + t * W * H, W, 0), "build")
            ck(lib.klt_hip_track(ctx, cur, nxt, C.byref(td), dx, dy, dv, NF, 1), "forward")
            for d, s in ((bx, dx), (by, dy), (bv, dv)):
                ck(lib.klt_hip_memcpy(ctx, d, s, 4 * NF, D2D), "copy")
            ck(lib.klt_hip_track(ctx, nxt, cur, C.byref(td), bx, by, bv, NF, 1), "backward")
            for d, a in ((dx, x1), (dy, y1), (dv, v1), (bx, xb), (by, yb), (bv, vb)):
                ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
            live = v1 >= 0
            ex, ey = xb - x, yb - y
            e = ex * ex + ey * ey
            rej = live & ((vb < 0) | (e > t2))
            x1[rej], y1[rej], v1[rej] = -1.0, -1.0, FB_REJECTED
            x, y, v = x1.copy(), y1.copy(), v1.copy()
            for d, a in ((dx, x), (dy, y), (dv, v)):
                ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
            cur = nxt
        ck(lib.klt_hip_sync(ctx), "sync")
        return time.perf_counter() - t0, (x, y, v)

    two_call()
    two = []
    for _ in range(args.rounds):
        dt, last = two_call()
        two.append(TT / dt)
    same = bool(np.array_equal(last[2], V[TT - 1]) and
                np.array_equal(last[0].view(np.int32), X[TT - 1].view(np.int32)) and
                np.array_equal(last[1].view(np.int32), Y[TT - 1].view(np.int32)))

    med = statistics.median
    out = {
        "tool": "fb_bench", "width": W, "height": H, "features": NF, "seed": args.seed, "frames": T,
        "chunk": args.chunk, "chunk_used": lib.klt_hip_frames_chunk(ctx), "rounds": args.rounds,
        "max_dist": args.max_dist,
        "fps_fb_off": [round(r, 1) for r in rate[False]], "fps_fb_on": [round(r, 1) for r in rate[True]],
        "fps_fb_off_median": round(med(rate[False]), 1), "fps_fb_on_median": round(med(rate[True]), 1),
        "fps_on_over_off": round(med(rate[True]) / med(rate[False]), 4),
        "tracker_us_per_frame_fb_off": [round(u, 3) for u in us[False]],
        "tracker_us_per_frame_fb_on": [round(u, 3) for u in us[True]],
        "tracker_us_on_over_off": round(med(us[True]) / med(us[False]), 3),
        "kernel_fb_off": kernel_off, "kernel_fb_on": kernel_fb,
        "rejected_total": int(new_rej.sum()), "rejected_per_frame": round(float(new_rej.sum()) / T, 3),
        "live_at_end_fb_off": live_off, "live_at_end_fb_on": live_on,
        "two_call_frames": TT, "two_call_fps": [round(r, 1) for r in two],
        "two_call_fps_median": round(med(two), 1),
        "fused_over_two_call": round(med(rate[True]) / med(two), 2),
        "two_call_equals_fused": same,
    }
    for d in (dfr, dx, dy, dv, tx, ty, tv, te, bx, by, bv):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
