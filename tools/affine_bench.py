#!/usr/bin/env python3
"""What the affine consistency check costs inside the batched tracker launch
(klt_hip_set_frames_affine), at bench.py's headline shape: 1080p, 5000 features
selected on frame 0, synthetic seed 1080, device-resident frames,
klt_hip_track_frames in 64-frame chunks, the default 15x15 affine window.

In one process, each leg from the same selection state over the same frames,
`--rounds` times, alternating:
  (a) the check off, on full level-0 records (klt_hip_set_lazy_grad 0);
  (b) the check inside the launch, modes 0, 1 and 2;
  (c) a loop of klt_hip_track_affine calls (mode 2) over the same frames -- one
      pyramid build and one host round trip per frame, which is what
      KLTTrackSequence amounted to before the check moved into the launch.
Frames/s over a host clock around the call and a device synchronise, and -- in
a replay of its own with events on -- the tracker's microseconds per frame
from klt_hip_get_timing.  (c)'s final list is checked against (b)'s mode 2.

With --parent-lib PATH (a libklt_amd.so built from the parent commit) it also
times KLTTrackSequence with mode 2 from host frames on that library and on this
tree's, alternating, `--seq-runs` fresh processes each (the library is chosen
when the process starts), and reports both medians and spreads.

Prints one JSON line.  Needs a GPU; there is no fallback.

  python tools/affine_bench.py [--frames 128] [--rounds 3] [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

AFF_RESET = (-1.0, -1.0, 1.0, 0.0, 0.0, 1.0)  # a fresh feature's affine fields


def affine_tc(tc, mode):
    tc.contents.affineConsistencyCheck = mode
    tc.contents.affine_window_width = tc.contents.affine_window_height = 15


def seq_child(args) -> None:
    """One process: KLTTrackSequence with mode 2 over host frames, a warm-up
    run and a timed one, each on a fresh selection.  Prints the seconds."""
    import kltamd
    from kltamd.device import D2H, check

    lib = kltamd.load()
    lib.KLTSetVerbosity(0)
    W, H, NF, T = args.width, args.height, args.features, args.seq_frames
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    affine_tc(tc, 2)
    ctx = lib.klt_amd_device_context(tc)
    dfr = lib.klt_hip_malloc(ctx, (T + 1) * W * H)
    check(lib, ctx, lib.klt_hip_synth_frames(ctx, args.seed, 0, T + 1, W, H, dfr, W, W * H), "synth")
    frames = np.empty((T + 1, H, W), np.uint8)
    check(lib, ctx, lib.klt_hip_memcpy(ctx, frames.ctypes.data, dfr, frames.nbytes, D2H), "frames")
    lib.klt_hip_free(ctx, dfr)
    U8P = C.POINTER(C.c_ubyte)
    arr = (U8P * (T + 1))(*[frames[t].ctypes.data_as(U8P) for t in range(T + 1)])
    out = []
    for _ in range(2):
        fl = lib.KLTCreateFeatureList(NF)
        lib.KLTSelectGoodFeatures(tc, arr[0], W, H, fl)
        lib.KLTStopSequentialMode(tc)  # every run starts from frames[0] itself
        t0 = time.perf_counter()
        lib.KLTTrackSequence(tc, arr, T + 1, W, H, fl, None, 0)
        out.append(time.perf_counter() - t0)
        live = lib.KLTCountRemainingFeatures(fl)
        held = sum(1 for k in range(NF) if fl.contents.feature[k].contents.aff_img)
        lib.KLTFreeFeatureList(fl)
    lib.KLTFreeTrackingContext(tc)
    print(json.dumps({"seconds": out[1], "warmup_seconds": out[0], "live": live, "held": held}))


def seq_compare(args) -> dict:
    this = str(ROOT / "klt-feature-tracker-acceleration-gpus_amd" / "lib" / "libklt_amd.so")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--seq-child", "--width", str(args.width), "--height",
           str(args.height), "--features", str(args.features), "--seed", str(args.seed), "--seq-frames",
           str(args.seq_frames)]
    res = {"parent": [], "this": []}
    for _ in range(args.seq_runs):
        for side, lib in (("parent", args.parent_lib), ("this", this)):
            p = subprocess.run(cmd, env={**os.environ, "KLT_AMD_LIB": lib}, capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"affine_bench: KLTTrackSequence child ({side}) failed:\n{p.stderr[-2000:]}")
            res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    T = args.seq_frames
    out = {"seq_frames": T, "seq_runs": args.seq_runs}
    for side in ("parent", "this"):
        fps = [T / r["seconds"] for r in res[side]]
        out[f"seq_fps_{side}"] = [round(f, 1) for f in fps]
        out[f"seq_fps_{side}_median"] = round(statistics.median(fps), 1)
        out[f"seq_fps_{side}_spread_pct"] = round(100.0 * (max(fps) - min(fps)) / statistics.median(fps), 2)
        out[f"seq_live_{side}"] = res[side][-1]["live"]
        out[f"seq_held_{side}"] = res[side][-1]["held"]
    out["seq_this_over_parent"] = round(out["seq_fps_this_median"] / out["seq_fps_parent_median"], 3)
    out["seq_same_result"] = bool(out["seq_live_parent"] == out["seq_live_this"] and
                                  out["seq_held_parent"] == out["seq_held_this"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=128, help="tracked frames per run")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=32, help="frames of the klt_hip_track_affine loop")
    ap.add_argument("--parent-lib", default=None, help="libklt_amd.so of the parent commit (KLTTrackSequence A/B)")
    ap.add_argument("--seq-frames", type=int, default=48, help="tracked frames of the KLTTrackSequence comparison")
    ap.add_argument("--seq-runs", type=int, default=5, help="processes per side of that comparison")
    ap.add_argument("--seq-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.seq_child:
        return seq_child(args)
    if args.rounds < 3:
        raise SystemExit("--rounds: at least 3")
    if args.seq_runs < 5:
        raise SystemExit("--seq-runs: at least 5")

    import kltamd
    from kltamd.device import D2H, H2D, AffineDesc, PyrDesc, Timing, TrackDesc, check

    lib = kltamd.load()
    if lib.klt_hip_device_count() <= 0:
        raise SystemExit("affine_bench: no HIP device visible")
    lib.KLTSetVerbosity(0)
    W, H, NF, T = args.width, args.height, args.features, args.frames
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    affine_tc(tc, 2)
    ctx = lib.klt_amd_device_context(tc)
    ck = lambda rc, what: check(lib, ctx, rc, what)  # noqa: E731

    dfr = lib.klt_hip_malloc(ctx, (T + 1) * W * H)
    ck(lib.klt_hip_synth_frames(ctx, args.seed, 0, T + 1, W, H, dfr, W, W * H), "synth")
    f0 = np.empty((H, W), np.uint8)
    ck(lib.klt_hip_memcpy(ctx, f0.ctypes.data, dfr, f0.nbytes, D2H), "frame 0")
    fl = lib.KLTCreateFeatureList(NF)
    lib.KLTSelectGoodFeatures(tc, f0.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, fl)
    x0 = np.array([fl.contents.feature[k].contents.x for k in range(NF)], np.float32)
    y0 = np.array([fl.contents.feature[k].contents.y for k in range(NF)], np.float32)
    v0 = np.array([fl.contents.feature[k].contents.val for k in range(NF)], np.int32)
    lib.KLTFreeFeatureList(fl)
    a0 = np.tile(np.array(AFF_RESET, np.float32), (NF, 1))
    s0 = np.zeros(NF, np.int32)
    dx, dy, dv, ds = (lib.klt_hip_malloc(ctx, 4 * NF) for _ in range(4))
    da = lib.klt_hip_malloc(ctx, 4 * 6 * NF)
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))
    ad = AffineDesc.from_tc(tc.contents)
    assert lib.klt_hip_affine_reserve(ctx, NF, ad.window_width, ad.window_height) >= 0
    ck(lib.klt_hip_set_lazy_grad(ctx, 0), "lazy off")  # every leg on full level-0 records

    def reset():
        for d, a in ((dx, x0), (dy, y0), (dv, v0), (ds, s0), (da, a0)):
            ck(lib.klt_hip_memcpy(ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")
        ck(lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr, W), "begin")
        ck(lib.klt_hip_set_track_order(ctx, 0), "order")  # no cached order carries over
        ck(lib.klt_hip_sync(ctx), "sync")

    def batched(mode, timing=False):
        """One run over the T frames (mode None: the check off); seconds, host clock, synchronised."""
        if mode is None:
            ck(lib.klt_hip_set_frames_affine(ctx, None, None, None), "off")
        else:
            ad.mode = mode
            ck(lib.klt_hip_set_frames_affine(ctx, C.byref(ad), da, ds), "on")
        reset()
        ck(lib.klt_hip_set_timing(ctx, 1 if timing else 0), "timing")
        t0 = time.perf_counter()
        rc = lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + W * H, W, W * H, T, args.chunk, dx, dy, dv,
                                      NF, None, None, None, 0)
        ck(lib.klt_hip_sync(ctx), "sync")
        dt = time.perf_counter() - t0
        ck(rc, "track_frames")
        return dt

    def final():
        x, y, v, s = np.empty(NF, np.float32), np.empty(NF, np.float32), np.empty(NF, np.int32), np.empty(NF, np.int32)
        a = np.empty((NF, 6), np.float32)
        for d, h in ((dx, x), (dy, y), (dv, v), (ds, s), (da, a)):
            ck(lib.klt_hip_memcpy(ctx, h.ctypes.data, d, h.nbytes, D2H), "d2h")
        return x, y, v, a, s

    legs = (None, 0, 1, 2)
    key = lambda m: "off" if m is None else f"mode{m}"  # noqa: E731
    w0 = time.perf_counter()
    while time.perf_counter() - w0 < 0.5:  # code objects, banks, the sustained clock
        for m in legs:
            batched(m)
    rate = {m: [] for m in legs}
    kernel, live, held = {}, {}, {}
    for _ in range(args.rounds):
        for m in legs:
            rate[m].append(T / batched(m))
            kernel[m] = lib.klt_hip_track_kernel(ctx).decode()
            _, _, v, _, s = final()
            live[m], held[m] = int((v >= 0).sum()), int((s != 0).sum())
    us = {m: [] for m in legs}
    tm = Timing()
    for _ in range(args.rounds):
        for m in legs:
            batched(m, timing=True)
            ck(lib.klt_hip_get_timing(ctx, C.byref(tm)), "timing")
            us[m].append(1e3 * tm.ms_track / max(1, tm.frames_track))
    ck(lib.klt_hip_set_timing(ctx, 0), "timing off")

    # (c) per frame: one pyramid, one klt_hip_track_affine call with host arrays
    TL = min(T, args.loop_frames)
    ad.mode = 2
    F, I = C.POINTER(C.c_float), C.POINTER(C.c_int)

    def loop():
        ck(lib.klt_hip_set_frames_affine(ctx, None, None, None), "off")
        assert lib.klt_hip_affine_reserve(ctx, NF, ad.window_width, ad.window_height) >= 0
        x, y, v, a, s = x0.copy(), y0.copy(), v0.copy(), a0.copy(), s0.copy()
        ck(lib.klt_hip_build_pyramid(ctx, 0, C.byref(pd), dfr, W, 0), "build")
        ck(lib.klt_hip_sync(ctx), "sync")
        cur = 0
        t0 = time.perf_counter()
        for t in range(1, TL + 1):
            nxt = 1 - cur
            ck(lib.klt_hip_build_pyramid(ctx, nxt, C.byref(pd), dfr + t * W * H, W, 0), "build")
            ck(lib.klt_hip_track_affine(ctx, cur, nxt, C.byref(td), C.byref(ad), x.ctypes.data_as(F),
                                        y.ctypes.data_as(F), v.ctypes.data_as(I), a.ctypes.data_as(F),
                                        s.ctypes.data_as(I), NF), "track_affine")
            cur = nxt
        return time.perf_counter() - t0, (x, y, v, a, s)

    loop()
    loop_rate = []
    for _ in range(args.rounds):
        dt, last = loop()
        loop_rate.append(TL / dt)
    # the batched mode-2 run over the same TL frames must end where the loop ends
    T_full, T = T, TL
    batched(2)
    T = T_full
    bx, by, bv, ba, bs = final()
    same = bool(np.array_equal(bv, last[2]) and np.array_equal(bx.view(np.int32), last[0].view(np.int32)) and
                np.array_equal(by.view(np.int32), last[1].view(np.int32)) and
                np.array_equal(ba.view(np.int32), last[3].view(np.int32)) and
                np.array_equal(bs != 0, last[4] != 0))

    med = statistics.median
    spread = lambda r: round(100.0 * (max(r) - min(r)) / med(r), 2)  # noqa: E731
    out = {"tool": "affine_bench", "width": W, "height": H, "features": NF, "seed": args.seed, "frames": T,
           "chunk": args.chunk, "chunk_used": lib.klt_hip_frames_chunk(ctx), "rounds": args.rounds,
           "affine_window": ad.window_width}
    for m in legs:
        k = key(m)
        out[f"fps_{k}"] = [round(r, 1) for r in rate[m]]
        out[f"fps_{k}_median"] = round(med(rate[m]), 1)
        out[f"fps_{k}_spread_pct"] = spread(rate[m])
        out[f"tracker_us_per_frame_{k}"] = [round(u, 3) for u in us[m]]
        out[f"tracker_us_per_frame_{k}_median"] = round(med(us[m]), 3)
        out[f"kernel_{k}"] = kernel[m]
        out[f"live_at_end_{k}"] = live[m]
        out[f"windows_held_at_end_{k}"] = held[m]
    out["loop_frames"] = TL
    out["loop_fps"] = [round(r, 1) for r in loop_rate]
    out["loop_fps_median"] = round(med(loop_rate), 1)
    out["batched_mode2_over_loop"] = round(med(rate[2]) / med(loop_rate), 2)
    out["loop_equals_batched"] = same
    for d in (dfr, dx, dy, dv, ds, da):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)
    if args.parent_lib:
        out.update(seq_compare(args))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
