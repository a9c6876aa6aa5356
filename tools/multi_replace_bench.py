#!/usr/bin/env python3
"""S independent sequences with lost features replaced every `every` frames:
one after another, or in one batched call.

  A  the S sequences one after another on one context, each with
     klt_hip_frames_begin + klt_hip_set_frames_replace + klt_hip_track_frames
     (what a caller had before klt_hip_track_frames_multi_replace: one small
     tracker launch, one small trackability map and one host round trip per
     sequence and replacement);
  B  one klt_hip_track_frames_multi_replace call over all of them (one tracker
     sub-launch, one list transfer and one map launch per replacement for all
     sequences; the selections still run one sequence after the other).

Device-resident synthetic frames (a seed per sequence, frame-major in one
buffer, which both sides read in place), start lists from KLTSelectGoodFeatures
on each sequence's frame 0, x | y | val in one device block, the same chunk on
both sides, no feature tables.  Per shape, S and `every`: one discarded run of
each side, then `--pairs` alternating A / B runs in one process, each from the
same start lists; the time is a host clock around the calls and a device
synchronise.  Reported: total frames/s (sequences x frames / seconds) of every
run, the medians, B over A, A's own spread (max over min of its runs: what "no
difference" means on this box), the replacements run and slots filled, and
whether B's final lists equal A's byte for byte (the tool fails when they do
not).

Prints one text row per case and, last, one JSON line with everything.  Needs a
GPU; there is no fallback.

  python tools/multi_replace_bench.py [--frames 100] [--pairs 7] [--chunk 25] [--every 1 5]
                                      [--shapes 320x240x150:1,4,16 ...]
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

DEFAULT_SHAPES = ["320x240x150:1,4,16", "640x480x1000:1,4,16"]


def parse_shape(text):
    dims, counts = text.split(":")
    w, h, nf = (int(v) for v in dims.split("x"))
    return w, h, nf, [int(v) for v in counts.split(",")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100, help="tracked frames per sequence")
    ap.add_argument("--pairs", type=int, default=7, help="alternating A / B runs per case (at least 5)")
    ap.add_argument("--chunk", type=int, default=25, help="frames per pyramid launch, both sides")
    ap.add_argument("--every", type=int, nargs="*", default=[1, 5], help="replace after every N-th tracked frame")
    ap.add_argument("--seed", type=int, default=1080, help="sequence s uses seed + s")
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES, help="WxHxFEATURES:S,S,...")
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("--pairs: at least 5")

    import kltamd
    from kltamd.device import D2H, H2D, PyrDesc, ReplaceDesc, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("multi_replace_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    T = args.frames
    rows = []
    print(f"# multi_replace_bench: {T} tracked frames per sequence, chunk {args.chunk}, {args.pairs} alternating pairs; "
          "frames/s = sequences x frames / seconds")
    print("# shape features S every | A median [min .. max] spread | B median [min .. max] | B/A | lists equal | "
          "replacements, slots filled | chunk A/B")
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
                raise SystemExit("multi_replace_bench: no device memory for the frames")
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
            n = S * NF
            start = np.concatenate([np.concatenate(x0).view(np.int32), np.concatenate(y0).view(np.int32),
                                    np.concatenate(v0)])
            dx = lib.klt_hip_malloc(ctx, 4 * 3 * n)  # x | y | val in one block
            dy, dv = dx + 4 * n, dx + 8 * n
            n_seq = (C.c_int * S)(*([NF] * S))
            pd, td = PyrDesc(), TrackDesc()
            lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
            lib.klt_amd_track_desc(tc, C.byref(td))
            for every in args.every:
                rd = ReplaceDesc.from_tc(tc.contents, every)
                chunk_seen, done = {}, {}

                def reset():
                    ck(lib.klt_hip_memcpy(ctx, dx, start.ctypes.data, start.nbytes, H2D), "h2d")
                    ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
                    ck(lib.klt_hip_sync(ctx), "sync")

                def lists():
                    a = np.empty(3 * n, np.int32)
                    ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, dx, a.nbytes, D2H), "d2h")
                    return a.tobytes()

                def side_a():
                    reset()
                    runs, filled = 0, 0
                    r, f = C.c_long(), C.c_long()
                    t0 = time.perf_counter()
                    for s in range(S):
                        o = 4 * s * NF
                        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr + s * fb, W), "begin")
                        ck(lib.klt_hip_set_frames_replace(ctx, C.byref(rd)), "replace on")
                        ck(lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + (S + s) * fb, W, S * fb, T,
                                                    args.chunk, dx + o, dy + o, dv + o, NF, None, None, None, 0), "frames")
                        ck(lib.klt_hip_get_frames_replace(ctx, None, None, C.byref(r), C.byref(f)), "get")
                        runs, filled = runs + r.value, filled + f.value
                    ck(lib.klt_hip_sync(ctx), "sync")
                    dt = time.perf_counter() - t0
                    ck(lib.klt_hip_set_frames_replace(ctx, None), "replace off")
                    chunk_seen["A"] = lib.klt_hip_frames_chunk(ctx)
                    done["A"] = (runs, filled)
                    return dt

                def side_b():
                    reset()
                    runs, filled = (C.c_long * S)(), (C.c_long * S)()
                    t0 = time.perf_counter()
                    ck(lib.klt_hip_track_frames_multi_replace(ctx, C.byref(pd), C.byref(td), C.byref(rd), 0, dfr, W,
                                                              S * fb, fb, S, T, args.chunk, n_seq, dx, dy, dv, None,
                                                              None, None, 0, None, runs, filled), "multi_replace")
                    ck(lib.klt_hip_sync(ctx), "sync")
                    dt = time.perf_counter() - t0
                    chunk_seen["B"] = lib.klt_hip_frames_chunk(ctx)
                    done["B"] = (sum(runs), sum(filled))
                    return dt

                side_a()  # discarded: code objects, banks, clocks
                side_b()
                fa, fbs = [], []
                for _ in range(args.pairs):
                    fa.append(S * T / side_a())
                    la = lists()
                    fbs.append(S * T / side_b())
                    lb = lists()
                equal = la == lb and done["A"] == done["B"]
                live = int((np.frombuffer(lb, np.int32)[2 * n:] >= 0).sum())
                med = statistics.median
                row = {"width": W, "height": H, "features": NF, "sequences": S, "frames": T, "every": every,
                       "chunk": args.chunk, "chunk_a": chunk_seen["A"], "chunk_b": chunk_seen["B"],
                       "fps_a": [round(v, 1) for v in fa], "fps_b": [round(v, 1) for v in fbs],
                       "fps_a_median": round(med(fa), 1), "fps_b_median": round(med(fbs), 1),
                       "b_over_a": round(med(fbs) / med(fa), 3), "a_spread": round(max(fa) / min(fa), 3),
                       "lists_equal": equal, "live_at_end": live, "replacements": done["B"][0],
                       "slots_filled": done["B"][1], "kernel_b": lib.klt_hip_track_kernel(ctx).decode(),
                       "map_kernel_b": lib.klt_hip_eigen_kernel(ctx).decode()}
                rows.append(row)
                print(f"{W}x{H} {NF:5d} S={S:2d} every={every:2d} | A {med(fa):10.1f} [{min(fa):10.1f} .. {max(fa):10.1f}] "
                      f"x{row['a_spread']:.3f} | B {med(fbs):10.1f} [{min(fbs):10.1f} .. {max(fbs):10.1f}] | "
                      f"B/A {row['b_over_a']:6.3f} | {'equal' if equal else 'DIFFERENT'} | {done['B'][0]}, {done['B'][1]} | "
                      f"{chunk_seen['A']}/{chunk_seen['B']}", flush=True)
            for d in (dfr, dx):
                lib.klt_hip_free(ctx, d)
            lib.KLTFreeTrackingContext(tc)
    print(json.dumps({"tool": "multi_replace_bench", "frames": T, "pairs": args.pairs, "chunk": args.chunk, "rows": rows}))
    if not all(r["lists_equal"] for r in rows):
        raise SystemExit("multi_replace_bench: B's lists or counters differ from A's")


if __name__ == "__main__":
    main()
