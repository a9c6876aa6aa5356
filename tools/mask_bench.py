#!/usr/bin/env python3
"""What the region mask (klt_hip_set_mask) costs on the device-resident batched
path.  An all-allowed mask changes no result, so both sides of each case do the
same work on the same frames and end with the same lists (checked).

  track    bench.py's headline shape -- 1080p, 5000 features selected on frame 0,
           synthetic seed 1080, klt_hip_track_frames in 64-frame chunks -- with an
           all-allowed tracking mask (KLT_HIP_MASK_TRACK: k_track7_mask_lazy, the
           lazy-gradient tracker with the test) against no mask, and -- with
           klt_hip_set_lazy_grad 0 on both sides -- k_track7_mask on full level-0
           records against the plain tracker on them;
  select   tools/replace_seq_bench.py's device-resident call, lost features
           replaced every 16 frames inside it, with an all-allowed selection mask
           (KLT_HIP_MASK_SELECT: one more byte read per map point in k_sel_init)
           against no mask.

Off and on alternate, `--rounds` times in one process after a discarded run of
each; the time is a host clock around the call and a device synchronise.  Per
side: every run, the median and the spread (max over min of its runs: what "no
difference" means on this box).  For the tracking case also the tracker's
microseconds per frame from klt_hip_get_timing, in runs of their own.

Writes the text rows and one JSON line to --out (default profiles/mask_ab.txt)
and to stdout; the committed profiles/mask_ab.txt holds a run's rows as its
second part, below the headline A/B of the setting off.  Needs a GPU; there is
no fallback.

  python tools/mask_bench.py [--frames 256] [--rounds 5] [--out profiles/mask_ab.txt]
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

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=256, help="tracked frames per run")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--every", type=int, default=16, help="replacement interval of the selection case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mask_ab.txt"))
    args = ap.parse_args()
    if args.rounds < 4:
        raise SystemExit("--rounds: at least 4")

    import kltamd
    from kltamd.device import D2H, H2D, MASK_SELECT, MASK_TRACK, PyrDesc, ReplaceDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("mask_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    W, H, NF, T = args.width, args.height, args.features, args.frames
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = lib.klt_amd_device_context(tc)
    ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731

    nfr = T + 1
    dfr = lib.klt_hip_malloc(ctx, nfr * W * H)
    if not dfr:
        raise SystemExit("mask_bench: no device memory for the frames")
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
    ones = np.ones((H, W), np.uint8)
    dmask = lib.klt_hip_malloc(ctx, ones.nbytes)
    ck(lib.klt_hip_memcpy(ctx, dmask, ones.ctypes.data, ones.nbytes, H2D), "mask")
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))

    def run(flags, on, every=0, timing=False, lazy=1):
        """One run over the T frames; returns seconds (host clock, synchronised) and the final lists' bytes."""
        ck(lib.klt_hip_set_lazy_grad(ctx, lazy), "lazy")
        ck(lib.klt_hip_set_mask(ctx, dmask if on else None, W, flags if on else 0), "set_mask")
        rd = ReplaceDesc.from_tc(tc.contents, every) if every else None
        ck(lib.klt_hip_set_frames_replace(ctx, C.byref(rd) if every else None), "replace")
        for d, a in ((dx, x0), (dy, y0), (dv, v0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
        ck(lib.klt_hip_set_timing(ctx, 1 if timing else 0), "timing")
        ck(lib.klt_hip_sync(ctx), "sync")
        t0 = time.perf_counter()
        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
        rc = lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + W * H, W, W * H, T, args.chunk, dx, dy, dv, NF,
                                      None, None, None, 0)
        ck(lib.klt_hip_sync(ctx), "sync")
        dt = time.perf_counter() - t0
        ck(rc, "track_frames")
        out = b""
        for d, dt_ in ((dx, np.float32), (dy, np.float32), (dv, np.int32)):
            a = np.empty(NF, dt_)
            ck(lib.klt_hip_memcpy(ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
            out += a.tobytes()
        return dt, out

    med = statistics.median
    lines = [f"# mask_bench: {W}x{H}, {NF} features, seed {args.seed}, {T} tracked frames in chunks of {args.chunk}, "
             f"{args.rounds} alternating rounds; frames/s",
             "# case | off median [min .. max] spread | on median [min .. max] spread | on/off | lists equal | kernels"]
    result = {"tool": "mask_bench", "width": W, "height": H, "features": NF, "seed": args.seed, "frames": T,
              "chunk": args.chunk, "rounds": args.rounds, "cases": []}
    for name, flags, every, lazy in (("track", MASK_TRACK, 0, 1), ("track_records", MASK_TRACK, 0, 0),
                                     ("select", MASK_SELECT, args.every, 1)):
        w0 = time.perf_counter()  # warm-up: both sides' code objects, the banks, the sustained clock
        while time.perf_counter() - w0 < 0.5:
            run(flags, False, every, lazy=lazy)
            run(flags, True, every, lazy=lazy)
        rate = {False: [], True: []}
        lists = {}
        kernel = {}
        for _ in range(args.rounds):
            for on in (False, True):
                dt, lists[on] = run(flags, on, every, lazy=lazy)
                rate[on].append(T / dt)
                kernel[on] = lib.klt_hip_track_kernel(ctx).decode()
        case = {"case": name, "every": every, "lazy_grad": lazy, "fps_off": [round(r, 1) for r in rate[False]],
                "fps_on": [round(r, 1) for r in rate[True]], "fps_off_median": round(med(rate[False]), 1),
                "fps_on_median": round(med(rate[True]), 1), "on_over_off": round(med(rate[True]) / med(rate[False]), 4),
                "off_spread": round(max(rate[False]) / min(rate[False]), 4),
                "on_spread": round(max(rate[True]) / min(rate[True]), 4), "lists_equal": lists[False] == lists[True],
                "kernel_off": kernel[False], "kernel_on": kernel[True]}
        if not every:  # the tracker's own time, events on (runs of their own)
            tm = Timing()
            for on in (False, True):
                vals = []
                for _ in range(args.rounds):
                    run(flags, on, every, timing=True, lazy=lazy)
                    ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
                    vals.append(1e3 * tm.ms_track / max(1, tm.frames_track))
                case["tracker_us_per_frame_on" if on else "tracker_us_per_frame_off"] = [round(u, 3) for u in vals]
            case["tracker_us_on_over_off"] = round(med(case["tracker_us_per_frame_on"]) /
                                                   med(case["tracker_us_per_frame_off"]), 3)
            ck(lib.klt_hip_set_timing(ctx, 0), "timing off")
        result["cases"].append(case)
        f, o = rate[False], rate[True]
        lines.append(f"{name:13s} | off {med(f):9.1f} [{min(f):9.1f} .. {max(f):9.1f}] x{case['off_spread']:.4f} | "
                     f"on {med(o):9.1f} [{min(o):9.1f} .. {max(o):9.1f}] x{case['on_spread']:.4f} | "
                     f"{case['on_over_off']:6.4f} | {'equal' if case['lists_equal'] else 'DIFFERENT'} | "
                     f"{kernel[False]} / {kernel[True]}")
        if not every:
            lines.append(f"              | tracker us per frame: off {med(case['tracker_us_per_frame_off']):.3f}, "
                         f"on {med(case['tracker_us_per_frame_on']):.3f}, on/off {case['tracker_us_on_over_off']:.3f}")
        print(lines[-1 if every else -2], flush=True)
    ck(lib.klt_hip_set_lazy_grad(ctx, 1), "lazy")
    ck(lib.klt_hip_set_mask(ctx, None, 0, 0), "mask off")
    ck(lib.klt_hip_set_frames_replace(ctx, None), "replace off")
    for d in (dfr, dx, dy, dv, dmask):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    lines.append(json.dumps(result))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text, end="")
    if not all(c["lists_equal"] for c in result["cases"]):
        raise SystemExit("mask_bench: the lists differ")


if __name__ == "__main__":
    main()
