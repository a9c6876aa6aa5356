#!/usr/bin/env python3
"""Lost features replaced every K frames: the per-call loop against one batched call.

  A  the loop: KLTTrackFeatures per frame (sequential mode), KLTReplaceLostFeatures
     after every `every`-th frame (what a caller had before KLTTrackSequenceReplace);
  B  one KLTTrackSequenceReplace call over the same host frames.

Host synthetic frames, the start list from KLTSelectGoodFeatures on frame 0, no
feature table.  Per `every`: one discarded run of each side, then `--pairs`
alternating A / B runs in one process, each on a fresh tracking context from
the same start list; the time is a host clock around the calls (both return
with the list on the host).  Reported: frames/s of every run, the medians, B
over A, A's own spread (max over min of its runs: what "no difference" means on
this box), and whether B's final list equals A's byte for byte.

Then the device-resident call (klt_hip_frames_begin + klt_hip_track_frames with
klt_hip_set_frames_replace on) on the same frames in device memory, with
klt_hip_set_lazy_grad 1 and 0 alternating: the map of an image-only level 0 by
k_min_eigen7_img against the map of full records by k_min_eigen7.  Per side the
wall clock of the call and, from klt_hip_get_timing in a further run of its own,
the map kernel's time per launch.

Prints one text row per case and, last, one JSON line with everything.  Needs a
GPU; there is no fallback.

  python tools/replace_seq_bench.py [--frames 256] [--pairs 7] [--every 1 4 16 64] [--shape 1920x1080x5000]
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
    ap.add_argument("--frames", type=int, default=256, help="tracked frames")
    ap.add_argument("--pairs", type=int, default=7, help="alternating A / B runs per case (at least 5)")
    ap.add_argument("--every", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--chunk", type=int, default=64, help="frames per launch of the device-resident call")
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--shape", default="1920x1080x5000", help="WxHxFEATURES")
    args = ap.parse_args()
    if args.pairs < 5:
        raise SystemExit("--pairs: at least 5")

    import kltamd
    from kltamd.abi import U8P
    from kltamd.device import H2D, D2H, PyrDesc, ReplaceDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("replace_seq_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    W, H, NF = (int(v) for v in args.shape.split("x"))
    T = args.frames
    frames = []
    for t in range(T + 1):
        a = np.empty((H, W), np.uint8)
        lib.klt_synth_frame(args.seed, t, W, H, a.ctypes.data)
        frames.append(a)
    ptr = [f.ctypes.data_as(U8P) for f in frames]
    arr = (U8P * (T + 1))(*ptr)

    tc0 = lib.KLTCreateTrackingContext()
    fl0 = lib.KLTCreateFeatureList(NF)
    lib.KLTSelectGoodFeatures(tc0, ptr[0], W, H, fl0)
    x0 = np.array([fl0.contents.feature[k].contents.x for k in range(NF)], np.float32)
    y0 = np.array([fl0.contents.feature[k].contents.y for k in range(NF)], np.float32)
    v0 = np.array([fl0.contents.feature[k].contents.val for k in range(NF)], np.int32)
    lib.KLTFreeTrackingContext(tc0)

    def fresh():
        tc = lib.KLTCreateTrackingContext()
        tc.contents.sequentialMode = 1
        for k in range(NF):
            f = fl0.contents.feature[k].contents
            f.x, f.y, f.val = float(x0[k]), float(y0[k]), int(v0[k])
        return tc

    def final():
        return b"".join(np.array([getattr(fl0.contents.feature[k].contents, f) for k in range(NF)], dt).tobytes()
                        for f, dt in (("x", np.float32), ("y", np.float32), ("val", np.int32)))

    def side_a(every):
        tc = fresh()
        t0 = time.perf_counter()
        for i in range(1, T + 1):
            lib.KLTTrackFeatures(tc, ptr[i - 1], ptr[i], W, H, fl0)
            if i % every == 0:
                lib.KLTReplaceLostFeatures(tc, ptr[i], W, H, fl0)
        dt = time.perf_counter() - t0
        out = final()
        lib.KLTFreeTrackingContext(tc)
        return dt, out

    def side_b(every):
        tc = fresh()
        t0 = time.perf_counter()
        lib.KLTTrackSequenceReplace(tc, arr, T + 1, W, H, fl0, None, 0, every)
        dt = time.perf_counter() - t0
        out = final()
        lib.KLTFreeTrackingContext(tc)
        return dt, out

    med = statistics.median
    rows, dev_rows = [], []
    print(f"# replace_seq_bench: {W}x{H}, {NF} features, seed {args.seed}, {T} tracked frames, {args.pairs} alternating "
          "pairs; frames/s")
    print("# every | A median [min .. max] spread | B median [min .. max] | B/A | lists equal | live at end")
    for every in args.every:
        side_a(every)  # discarded: code objects, banks, clocks
        side_b(every)
        fa, fb = [], []
        for _ in range(args.pairs):
            dt, la = side_a(every)
            fa.append(T / dt)
            dt, lb = side_b(every)
            fb.append(T / dt)
        live = int((np.frombuffer(lb[8 * NF:], np.int32) >= 0).sum())
        row = {"every": every, "fps_a": [round(v, 1) for v in fa], "fps_b": [round(v, 1) for v in fb],
               "fps_a_median": round(med(fa), 1), "fps_b_median": round(med(fb), 1),
               "b_over_a": round(med(fb) / med(fa), 3), "a_spread": round(max(fa) / min(fa), 3),
               "lists_equal": la == lb, "live_at_end": live}
        rows.append(row)
        print(f"every {every:3d} | A {med(fa):9.1f} [{min(fa):9.1f} .. {max(fa):9.1f}] x{row['a_spread']:.3f} | "
              f"B {med(fb):9.1f} [{min(fb):9.1f} .. {max(fb):9.1f}] | B/A {row['b_over_a']:6.3f} | "
              f"{'equal' if la == lb else 'DIFFERENT'} | {live}", flush=True)

    # the device-resident call, lazy gradients on and off
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = lib.klt_amd_device_context(tc)
    ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731
    fbytes = W * H
    dfr = lib.klt_hip_malloc(ctx, (T + 1) * fbytes)
    if not dfr:
        raise SystemExit("replace_seq_bench: no device memory for the frames")
    ck(lib.klt_hip_synth_frames(ctx, args.seed, 0, T + 1, W, H, dfr, W, fbytes), "synth")
    dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(3))
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))

    def device_side(every, lazy, timing=False):
        ck(lib.klt_hip_set_lazy_grad(ctx, lazy), "lazy")
        for d, a in ((dx, x0), (dy, y0), (dv, v0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
        rd = ReplaceDesc.from_tc(tc.contents, every)
        ck(lib.klt_hip_set_frames_replace(ctx, C.byref(rd)), "replace")
        ck(lib.klt_hip_set_timing(ctx, 1 if timing else 0), "timing")
        ck(lib.klt_hip_sync(ctx), "sync")
        t0 = time.perf_counter()
        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
        ck(lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + fbytes, W, fbytes, T, args.chunk, dx, dy, dv, NF,
                                    None, None, None, 0), "frames")
        ck(lib.klt_hip_sync(ctx), "sync")
        dt = time.perf_counter() - t0
        runs = C.c_long()
        ck(lib.klt_hip_get_frames_replace(ctx, None, None, C.byref(runs), None), "get")
        tm = Timing()
        if timing:
            ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
        out = b""
        for d, dt_ in ((dx, np.float32), (dy, np.float32), (dv, np.int32)):
            a = np.empty(NF, dt_)
            ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
            out += a.tobytes()
        return dt, out, runs.value, tm, lib.klt_hip_eigen_kernel(ctx).decode()

    print("# device-resident call: every | lazy (k_min_eigen7_img) median ms [min .. max] spread | records "
          "(completion-free full level 0 + k_min_eigen7) median ms | records/lazy | map kernel us per launch lazy / "
          "records (generic-kernel us per replacement) | lists equal")
    for every in args.every:
        device_side(every, 1)
        device_side(every, 0)
        ta, tb = [], []
        for _ in range(args.pairs):
            dt, la, runs, _, _ = device_side(every, 1)
            ta.append(dt * 1e3)
            dt, lb, _, _, _ = device_side(every, 0)
            tb.append(dt * 1e3)
        _, _, _, t1, k1 = device_side(every, 1, timing=True)
        _, _, _, t0_, k0 = device_side(every, 0, timing=True)
        us = lambda t: round(1e3 * t.ms_eigen / t.n_eigen, 2) if t.n_eigen else None  # noqa: E731
        row = {"every": every, "replacements": runs, "ms_lazy": [round(v, 2) for v in ta],
               "ms_records": [round(v, 2) for v in tb], "ms_lazy_median": round(med(ta), 2),
               "ms_records_median": round(med(tb), 2), "records_over_lazy": round(med(tb) / med(ta), 3),
               "lazy_spread": round(max(ta) / min(ta), 3), "map_us_lazy": us(t1), "map_us_records": us(t0_),
               "map_launches_lazy": t1.n_eigen, "map_launches_records": t0_.n_eigen,
               "generic_launches_lazy": t1.n_generic, "kernel_lazy": k1, "kernel_records": k0, "lists_equal": la == lb}
        dev_rows.append(row)
        print(f"every {every:3d} ({runs} replacements) | lazy {med(ta):9.2f} [{min(ta):9.2f} .. {max(ta):9.2f}] "
              f"x{row['lazy_spread']:.3f} | records {med(tb):9.2f} | {row['records_over_lazy']:6.3f} | "
              f"{row['map_us_lazy']} / {row['map_us_records']} us | {'equal' if la == lb else 'DIFFERENT'} | "
              f"{k1} / {k0}", flush=True)
    ck(lib.klt_hip_set_frames_replace(ctx, None), "replace off")
    for d in (dfr, dx, dy, dv):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    lib.KLTFreeFeatureList(fl0)
    print(json.dumps({"tool": "replace_seq_bench", "width": W, "height": H, "features": NF, "frames": T,
                      "pairs": args.pairs, "rows": rows, "device_rows": dev_rows}))
    if not all(r["lists_equal"] for r in rows + dev_rows):
        raise SystemExit("replace_seq_bench: the lists differ")


if __name__ == "__main__":
    main()
