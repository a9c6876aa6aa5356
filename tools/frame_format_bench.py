#!/usr/bin/env python3
"""Colour device frames: convert first, or let the level-0 kernel convert.

  A  klt_hip_to_gray over the frames (one call, into a gray buffer), then the
     gray klt_hip_frames_begin + klt_hip_track_frames on that buffer -- what a
     caller holding RGB/BGR(A) frames had to do before klt_hip_set_frame_format
     (with the library's own conversion kernel standing in for theirs);
  B  klt_hip_set_frame_format, then klt_hip_frames_begin + klt_hip_track_frames
     on the colour frames themselves.

Device-resident frames: synthetic gray frames f made on the device, turned into
colour with torch (R = (f >> 1) + 31, G = f, B = lut[f], alpha 255: the recipe
of tests/test_gpu_frame_format.py), a start list from KLTSelectGoodFeatures on
the converted frame 0, the same chunk on both sides, no feature tables.  Per
shape and format: one discarded run of each side, then `--pairs` alternating A /
B runs in one process, each from the same start list; the time is a host clock
around the calls and a device synchronise.  Reported: frames/s of every run, the
medians, B over A, A's own spread (max over min of its runs: what "no
difference" means on this box), whether B's final list equals A's byte for
byte, and from klt_hip_get_timing in one further run of each side the level-0
kernel's time per frame (the pyr_l0 class: k_pyr_l0 on A, k_pyr_l0_px on B).

Prints one text row per case and, last, one JSON line with everything.  Needs a
GPU and torch; there is no fallback.

  python tools/frame_format_bench.py [--frames 128] [--pairs 7] [--chunk 64]
        [--shapes 1920x1080x5000 3840x2160x20000] [--formats rgb8 rgba8]
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

FORMATS = {"rgb8": 1, "bgr8": 2, "rgba8": 3, "bgra8": 4}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128, help="tracked frames")
    ap.add_argument("--pairs", type=int, default=7, help="alternating A / B runs per case (at least 5)")
    ap.add_argument("--chunk", type=int, default=64, help="frames per launch, both sides")
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--shapes", nargs="*", default=["1920x1080x5000", "3840x2160x20000"], help="WxHxFEATURES")
    ap.add_argument("--formats", nargs="*", default=["rgb8", "rgba8"], choices=sorted(FORMATS))
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("--pairs: at least 5")

    import torch

    import kltamd
    from kltamd.device import D2H, H2D, PyrDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0 or not torch.cuda.is_available():
        raise SystemExit("frame_format_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    T = args.frames
    dev = torch.device("cuda", lib.klt_hip_current_device())
    lut = torch.from_numpy(np.random.default_rng(2024).permutation(256).astype(np.uint8)).to(dev)
    rows = []
    print(f"# frame_format_bench: {T} tracked frames, chunk {args.chunk}, {args.pairs} alternating pairs")
    print("# shape features format | A median [min .. max] spread | B median [min .. max] | B/A | lists equal | "
          "pyr_l0 us/frame A, B | to_gray us/frame")
    for shape in args.shapes:
        W, H, NF = (int(v) for v in shape.split("x"))
        for name in args.formats:
            fmt = FORMATS[name]
            bpp = lib.klt_hip_frame_bpp(fmt)
            tc = lib.KLTCreateTrackingContext()
            tc.contents.sequentialMode = 1
            ctx = lib.klt_amd_device_context(tc)
            ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731
            fb = W * H
            gray = torch.empty((T + 1, H, W), dtype=torch.uint8, device=dev)  # A's converted frames
            col = torch.empty((T + 1, H, W, bpp), dtype=torch.uint8, device=dev)
            ck(lib.klt_hip_synth_frames(ctx, args.seed, 0, T + 1, W, H, gray.data_ptr(), W, fb), "synth")
            ck(lib.klt_hip_sync(ctx), "sync")
            for t in range(T + 1):  # frame by frame: the index tensor of a whole 4K sequence would not fit
                f = gray[t]
                r, b = (f >> 1) + 31, lut[f.long()]
                col[t, ..., 0], col[t, ..., 1], col[t, ..., 2] = (b, f, r) if fmt in (2, 4) else (r, f, b)
                if bpp == 4:
                    col[t, ..., 3] = 255
            torch.cuda.synchronize(dev)
            gptr, cptr, pitch = gray.data_ptr(), col.data_ptr(), W * bpp

            def to_gray():
                ck(lib.klt_hip_to_gray(ctx, fmt, cptr, pitch, pitch * H, T + 1, W, H, gptr, W, fb), "to_gray")

            to_gray()
            f0 = np.empty((H, W), np.uint8)
            ck(lib.klt_hip_sync(ctx), "sync")
            ck(lib.klt_hip_memcpy(ctx, f0.ctypes.data, gptr, f0.nbytes, D2H), "frame 0")
            fl = lib.KLTCreateFeatureList(NF)
            lib.KLTSelectGoodFeatures(tc, f0.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, fl)
            x0 = np.array([fl.contents.feature[k].contents.x for k in range(NF)], np.float32)
            y0 = np.array([fl.contents.feature[k].contents.y for k in range(NF)], np.float32)
            v0 = np.array([fl.contents.feature[k].contents.val for k in range(NF)], np.int32)
            lib.KLTFreeFeatureList(fl)
            dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(3))
            pd, td = PyrDesc(), TrackDesc()
            lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
            lib.klt_amd_track_desc(tc, C.byref(td))

            def reset():
                for d, a in ((dx, x0), (dy, y0), (dv, v0)):
                    ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
                ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
                ck(lib.klt_hip_sync(ctx), "sync")

            def lists():
                out = []
                for d, dt in ((dx, np.float32), (dy, np.float32), (dv, np.int32)):
                    a = np.empty(NF, dt)
                    ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
                    out.append(a.tobytes())
                return out

            def track(f, ptr, p):
                ck(lib.klt_hip_set_frame_format(ctx, f), "format")
                ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), ptr, p), "begin")
                ck(lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), ptr + p * H, p, p * H, T, args.chunk, dx, dy,
                                            dv, NF, None, None, None, 0), "frames")

            def side_a():
                reset()
                gray.zero_()  # A starts without the converted frames
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                to_gray()
                track(0, gptr, W)
                ck(lib.klt_hip_sync(ctx), "sync")
                return time.perf_counter() - t0

            def side_b():
                reset()
                t0 = time.perf_counter()
                track(fmt, cptr, pitch)
                ck(lib.klt_hip_sync(ctx), "sync")
                return time.perf_counter() - t0

            def l0_us(side):
                ck(lib.klt_hip_set_timing(ctx, 1), "timing")
                side()
                tm = Timing()
                ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
                ck(lib.klt_hip_set_timing(ctx, 0), "timing")
                return 1e3 * tm.ms_pyr_l0 / max(tm.frames_pyr_l0, 1)

            def to_gray_us():
                ck(lib.klt_hip_sync(ctx), "sync")
                t0 = time.perf_counter()
                for _ in range(5):
                    to_gray()
                ck(lib.klt_hip_sync(ctx), "sync")
                return 1e6 * (time.perf_counter() - t0) / (5 * (T + 1))

            side_a()  # discarded: code objects, banks, clocks
            side_b()
            fa, fbs = [], []
            for _ in range(args.pairs):
                fa.append(T / side_a())
                la = lists()
                fbs.append(T / side_b())
                lb = lists()
            equal = la == lb
            us_a, us_b, us_g = l0_us(side_a), l0_us(side_b), to_gray_us()
            med = statistics.median
            row = {"width": W, "height": H, "features": NF, "format": name, "frames": T, "chunk": args.chunk,
                   "chunk_used": lib.klt_hip_frames_chunk(ctx),
                   "fps_a": [round(v, 1) for v in fa], "fps_b": [round(v, 1) for v in fbs],
                   "fps_a_median": round(med(fa), 1), "fps_b_median": round(med(fbs), 1),
                   "b_over_a": round(med(fbs) / med(fa), 3), "a_spread": round(max(fa) / min(fa), 3),
                   "pyr_l0_us_per_frame_a": round(us_a, 2), "pyr_l0_us_per_frame_b": round(us_b, 2),
                   "to_gray_us_per_frame": round(us_g, 2), "lists_equal": equal,
                   "live_at_end": int((np.frombuffer(lb[2], np.int32) >= 0).sum())}
            rows.append(row)
            print(f"{W}x{H} {NF:5d} {name:5s} | A {med(fa):9.1f} [{min(fa):9.1f} .. {max(fa):9.1f}] x{row['a_spread']:.3f}"
                  f" | B {med(fbs):9.1f} [{min(fbs):9.1f} .. {max(fbs):9.1f}] | B/A {row['b_over_a']:6.3f}"
                  f" | {'equal' if equal else 'DIFFERENT'} | {us_a:6.2f} {us_b:6.2f} | {us_g:6.2f}", flush=True)
            for d in (dx, dy, dv):
                lib.klt_hip_free(ctx, d)
            lib.KLTFreeTrackingContext(tc)
            del gray, col
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "frame_format_bench", "frames": T, "pairs": args.pairs, "chunk": args.chunk,
                      "rows": rows}))
    if not all(r["lists_equal"] for r in rows):
        raise SystemExit("frame_format_bench: B's list differs from A's")


if __name__ == "__main__":
    main()
