#!/usr/bin/env python3
"""S independent sequences on one GPU: one after another, or in one batched call.

  A  the S sequences tracked one after another on one context, each with
     klt_hip_frames_begin + klt_hip_track_frames (what a caller had before
     klt_hip_track_frames_multi);
  B  one klt_hip_track_frames_multi call over all of them.

Device-resident synthetic frames (a seed per sequence, frame-major in one
buffer, which both sides read in place), start lists from KLTSelectGoodFeatures
on each sequence's frame 0, the same chunk on both sides, no feature tables.
Per shape and S: one discarded warm-up of each side, then `--pairs` alternating
A / B runs in one process, each from the same start lists; the time is a host
clock around the calls and a device synchronise.  Reported: total frames/s
(sequences x frames / seconds) of every run, the medians, B over A, A's own
spread (max over min of its runs: what "no difference" means on this box), and
whether B's final lists equal A's byte for byte.  At S = 1 a third side joins the
alternation: A with klt_hip_set_lazy_grad 0, i.e. on the full level-0 records
that B's banks hold -- it separates what the bank layout costs or saves from
what the batching does.

Prints one text row per case and, last, one JSON line with everything.  Needs a
GPU; there is no fallback.

  python tools/multi_bench.py [--frames 100] [--pairs 7] [--chunk 25] [--shapes 320x240x150:1,2,4,8,16 ...]
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

DEFAULT_SHAPES = ["320x240x150:1,2,4,8,16", "640x480x1000:1,2,4,8,16", "1920x1080x5000:1,2,4,8"]


def parse_shape(text):
    dims, counts = text.split(":")
    w, h, nf = (int(v) for v in dims.split("x"))
    return w, h, nf, [int(v) for v in counts.split(",")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100, help="tracked frames per sequence")
    ap.add_argument("--pairs", type=int, default=7, help="alternating A / B runs per case (at least 5)")
    ap.add_argument("--chunk", type=int, default=25, help="frames per launch, both sides")
    ap.add_argument("--seed", type=int, default=1080, help="sequence s uses seed + s")
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES, help="WxHxFEATURES:S,S,...")
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("--pairs: at least 5")

    import kltamd
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("multi_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    T = args.frames
    rows = []
    print(f"# multi_bench: {T} tracked frames per sequence, chunk {args.chunk}, {args.pairs} alternating pairs; "
          "frames/s = sequences x frames / seconds")
    print("# shape features S | A median [min .. max] spread | B median [min .. max] | B/A | lists equal | chunk A/B")
    for shape in args.shapes:
        W, H, NF, counts = parse_shape(shape)
        for S in counts:
            tc = lib.KLTCreateTrackingContext()
            tc.contents.sequentialMode = 1
            ctx = lib.klt_amd_device_context(tc)
            ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731
            fb = W * H
            dfr = lib.klt_hip_malloc(ctx, (T + 1) * S * fb)  # frame f of sequence s at (f * S + s) * fb
            if not dfr:
                raise SystemExit("multi_bench: no device memory for the frames")
            x0, y0, v0 = [], [], []
            f0 = np.empty((H, W), np.uint8)
            for s in range(S):
                ck(lib.klt_hip_synth_frames(ctx, args.seed + s, 0, T + 1, W, H, dfr + s * fb, W, S * fb), "synth")
                ck(lib.klt_hip_memcpy(ctx, f0.ctypes.data, dfr + s * fb, f0.nbytes, D2H), "frame 0")
                fl = lib.KLTCreateFeatureList(NF)
                lib.KLTSelectGoodFeatures(tc, f0.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, fl)
                x0.append(np.array([fl.contents.feature[k].contents.x for k in range(NF)], np.float32))
                y0.append(np.array([fl.contents.feature[k].contents.y for k in range(NF)], np.float32))
                v0.append(np.array([fl.contents.feature[k].contents.val for k in range(NF)], np.int32))
                lib.KLTFreeFeatureList(fl)
            x0, y0, v0 = np.concatenate(x0), np.concatenate(y0), np.concatenate(v0)
            n = S * NF
            dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * n) for _ in range(3))
            n_seq = (C.c_int * S)(*([NF] * S))
            pd, td = PyrDesc(), TrackDesc()
            lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
            lib.klt_amd_track_desc(tc, C.byref(td))
            chunk_seen = {}

            def reset():
                for d, a in ((dx, x0), (dy, y0), (dv, v0)):
                    ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
                ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
                ck(lib.klt_hip_sync(ctx), "sync")

            def lists():
                out = []
                for d, dt in ((dx, np.float32), (dy, np.float32), (dv, np.int32)):
                    a = np.empty(n, dt)
                    ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
                    out.append(a.tobytes())
                return out

            def side_a(lazy=1):
                ck(lib.klt_hip_set_lazy_grad(ctx, lazy), "lazy")
                reset()
                t0 = time.perf_counter()
                for s in range(S):
                    o = 4 * s * NF
                    ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr + s * fb, W), "begin")
                    ck(lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + (S + s) * fb, W, S * fb, T,
                                                args.chunk, dx + o, dy + o, dv + o, NF, None, None, None, 0), "frames")
                ck(lib.klt_hip_sync(ctx), "sync")
                dt = time.perf_counter() - t0
                chunk_seen["A"] = lib.klt_hip_frames_chunk(ctx)
                return dt

            def side_b():
                reset()
                t0 = time.perf_counter()
                ck(lib.klt_hip_track_frames_multi(ctx, C.byref(pd), C.byref(td), dfr, W, S * fb, fb, S, T, args.chunk,
                                                  n_seq, dx, dy, dv, None, None, None, 0), "multi")
                ck(lib.klt_hip_sync(ctx), "sync")
                dt = time.perf_counter() - t0
                chunk_seen["B"] = lib.klt_hip_frames_chunk(ctx)
                return dt

            side_a()  # discarded: code objects, banks, clocks
            side_b()
            fa, fbs, far = [], [], []
            if S == 1:
                side_a(lazy=0)
            for _ in range(args.pairs):
                if S == 1:
                    far.append(S * T / side_a(lazy=0))
                fa.append(S * T / side_a())
                la = lists()
                fbs.append(S * T / side_b())
                lb = lists()
            equal = la == lb
            live = int((np.frombuffer(lb[2], np.int32) >= 0).sum())
            med = statistics.median
            row = {"width": W, "height": H, "features": NF, "sequences": S, "frames": T, "chunk": args.chunk,
                   "chunk_a": chunk_seen["A"], "chunk_b": chunk_seen["B"],
                   "fps_a": [round(v, 1) for v in fa], "fps_b": [round(v, 1) for v in fbs],
                   "fps_a_median": round(med(fa), 1), "fps_b_median": round(med(fbs), 1),
                   "b_over_a": round(med(fbs) / med(fa), 3), "a_spread": round(max(fa) / min(fa), 3),
                   "fps_a_records": [round(v, 1) for v in far],
                   "fps_a_records_median": round(med(far), 1) if far else None,
                   "b_over_a_records": round(med(fbs) / med(far), 3) if far else None,
                   "lists_equal": equal, "live_at_end": live,
                   "kernel_b": lib.klt_hip_track_kernel(ctx).decode()}
            rows.append(row)
            print(f"{W}x{H} {NF:5d} S={S:2d} | A {med(fa):10.1f} [{min(fa):10.1f} .. {max(fa):10.1f}] x{row['a_spread']:.3f}"
                  f" | B {med(fbs):10.1f} [{min(fbs):10.1f} .. {max(fbs):10.1f}] | B/A {row['b_over_a']:6.3f}"
                  f" | {'equal' if equal else 'DIFFERENT'} | {chunk_seen['A']}/{chunk_seen['B']}"
                  + (f" | A on full records {med(far):10.1f}, B over it {row['b_over_a_records']:.3f}" if far else ""),
                  flush=True)
            for d in (dfr, dx, dy, dv):
                lib.klt_hip_free(ctx, d)
            lib.KLTFreeTrackingContext(tc)
    print(json.dumps({"tool": "multi_bench", "frames": T, "pairs": args.pairs, "chunk": args.chunk, "rows": rows}))
    if not all(r["lists_equal"] for r in rows):
        raise SystemExit("multi_bench: B's lists differ from A's")


if __name__ == "__main__":
    main()
