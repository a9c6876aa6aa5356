#!/usr/bin/env python3
"""When do the waves of one lazy-gradient k_track7 launch leave the chip?

One klt_hip_track_frames call of one chunk (so: pyramids, then the tracker, on
one stream) with klt_hip_set_wave_times on, after the same call repeated
untimed from the same selection until the chip holds its sustained clock.  Prints
the entry and exit time distributions of the launch's waves, the share of the
resident wave slots that stood empty over the launch's length

    idle = 1 - sum(wave durations) / (min(waves, 5 * 1024) * launch length)

and idle x launch length: what building the next chunk in the tracker's tail
could save per chunk at the very most (a build that loses nothing by running
beside the last waves).  Also how long before the launch's end only K waves
were still running, for the K values klt_hip_set_frames_tail might take.

Every time carries the XCD its wave ran on (klt_hip_set_wave_times), so the
same figures are also given per XCD ("per_xcd"): its waves, how many of them
left within the first 5 us of the launch (lost features, padding slots), the
median and the last exit, and the idle share of its own slots (5 x 128) over
the whole launch's length.  --start-frame J measures the launch that begins
at frame J from the list as it stands after J tracked frames (tracked once,
untimed), when part of the list is lost: with the lost features last in the
processing order whole XCDs stand empty, with the balanced order
(KLT_ORDER_BALANCE=0 restores the former) none should.

    python tools/wave_tail.py --width 1920 --height 1080 --features 5000
    python tools/wave_tail.py --start-frame 448
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

TICK_US = 0.01  # wall_clock64(): 100 MHz
XCD_SHIFT, XCDS, SIMDS_PER_XCD = 60, 8, 128  # bits 60..63 of a time: the wave's XCD
EARLY_US = 5.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--warm", type=int, default=60, help="untimed calls before the measured ones")
    ap.add_argument("--runs", type=int, default=1, help="measured launches (one line each)")
    ap.add_argument("--seed", type=int, default=1080)
    ap.add_argument("--start-frame", type=int, default=0,
                    help="measure the chunk after this many tracked frames, from the list as it stands then")
    a = ap.parse_args()
    import kltamd
    from kltamd.device import D2H, H2D, PyrDesc, TrackDesc, check
    lib = kltamd.load()
    lib.KLTSetVerbosity(0)
    W, H, N, F, J = a.width, a.height, a.features, a.chunk, a.start_frame
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    ctx = lib.klt_amd_device_context(tc)
    nfr = 1 + J + F
    dfr = lib.klt_hip_malloc(ctx, nfr * W * H)
    check(lib, ctx, lib.klt_hip_synth_frames(ctx, a.seed, 0, nfr, W, H, dfr, W, W * H), "synth")
    f0 = np.empty((H, W), np.uint8)
    check(lib, ctx, lib.klt_hip_memcpy(ctx, f0.ctypes.data, dfr, f0.nbytes, D2H), "d2h")
    fl = lib.KLTCreateFeatureList(N)
    lib.KLTSelectGoodFeatures(tc, f0.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, fl)
    x = np.array([fl.contents.feature[k].contents.x for k in range(N)], np.float32)
    y = np.array([fl.contents.feature[k].contents.y for k in range(N)], np.float32)
    v = np.array([fl.contents.feature[k].contents.val for k in range(N)], np.int32)
    lib.KLTFreeFeatureList(fl)
    dx, dy, dv = (lib.klt_hip_malloc(ctx, 4 * N) for _ in range(3))
    pd, td = PyrDesc(), TrackDesc()
    lib.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(pd))
    lib.klt_amd_track_desc(tc, C.byref(td))
    cap = 8 * ((N + 31) // 32) * 4 + 64  # the launch's grid in XCD-major order, in waves, and some
    buf = np.zeros(4 + 2 * cap, np.uint64)
    dbuf = lib.klt_hip_malloc(ctx, buf.nbytes)

    def call(j0=J, nf=F):
        """frames j0+1..j0+nf from the start list on frame j0, every time"""
        for d, h in ((dx, x), (dy, y), (dv, v)):
            check(lib, ctx, lib.klt_hip_memcpy(ctx, d, h.ctypes.data, h.nbytes, H2D), "h2d")
        check(lib, ctx, lib.klt_hip_frames_begin(ctx, C.byref(pd), dfr + j0 * W * H, W), "begin")
        check(lib, ctx, lib.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + (j0 + 1) * W * H, W, W * H, nf,
                                                 F, dx, dy, dv, N, None, None, None, 0), "frames")

    if J > 0:  # the start list becomes the selection tracked through frames 1..J
        call(0, J)
        check(lib, ctx, lib.klt_hip_sync(ctx), "sync")
        for d, h in ((dx, x), (dy, y), (dv, v)):
            check(lib, ctx, lib.klt_hip_memcpy(ctx, h.ctypes.data, d, h.nbytes, D2H), "d2h")
    live = int((v >= 0).sum())

    for k in range(a.warm):
        call()
    check(lib, ctx, lib.klt_hip_sync(ctx), "sync")
    for r in range(a.runs):
        buf[:] = 0
        buf[2] = cap
        check(lib, ctx, lib.klt_hip_memcpy(ctx, dbuf, buf.ctypes.data, buf.nbytes, H2D), "h2d")
        check(lib, ctx, lib.klt_hip_set_wave_times(ctx, dbuf), "wave times on")
        call()
        check(lib, ctx, lib.klt_hip_sync(ctx), "sync")
        check(lib, ctx, lib.klt_hip_set_wave_times(ctx, None), "wave times off")
        check(lib, ctx, lib.klt_hip_memcpy(ctx, buf.ctypes.data, dbuf, buf.nbytes, D2H), "d2h")
        # entry times stand at the wave's number in the grid, exit times at its feature's
        # index (its slot when that holds no feature): not paired; a place no wave wrote is 0
        raw_in, raw_out = buf[4:4 + cap], buf[4 + cap:4 + 2 * cap]
        raw_in, raw_out = raw_in[raw_in != 0], raw_out[raw_out != 0]
        nin, nout = len(raw_in), len(raw_out)
        assert 0 < nin == nout, (nin, nout, cap)
        mask = np.uint64((1 << XCD_SHIFT) - 1)
        x_in, x_out = (raw_in >> np.uint64(XCD_SHIFT)).astype(np.int64), (raw_out >> np.uint64(XCD_SHIFT)).astype(np.int64)
        o_in, o_out = np.argsort(raw_in & mask, kind="stable"), np.argsort(raw_out & mask, kind="stable")
        t_in, x_in = (raw_in & mask).astype(np.int64)[o_in], x_in[o_in]
        t_out, x_out = (raw_out & mask).astype(np.int64)[o_out], x_out[o_out]
        t0, t1 = int(t_in[0]), int(t_out[-1])
        length = (t1 - t0) * TICK_US
        busy = float(t_out.sum() - t_in.sum()) * TICK_US
        slots = min(nin, 5 * 1024)
        idle = 1.0 - busy / (slots * length)
        end = (t_out - t0) * TICK_US
        q = lambda p: float(np.percentile(end, p))  # noqa: E731
        left = {}
        for K in (256, 512, 1024, 2048, 4096):
            if K < nout:
                left[K] = round(length - float(end[nout - K - 1]), 1)  # from "K waves left" to the end
        per_xcd = []
        for xc in range(XCDS):
            ti, to = t_in[x_in == xc], t_out[x_out == xc]
            assert len(ti) == len(to), (xc, len(ti), len(to))
            if not len(to):
                per_xcd.append({"xcd": xc, "waves": 0})
                continue
            ex = (to - t0) * TICK_US
            sl = min(len(to), 5 * SIMDS_PER_XCD)
            per_xcd.append({"xcd": xc, "waves": len(to), "left_in_first_5us": int((ex < EARLY_US).sum()),
                            "median_exit_us": round(float(np.median(ex)), 1), "last_exit_us": round(float(ex[-1]), 1),
                            "idle_share": round(1.0 - float(to.sum() - ti.sum()) * TICK_US / (sl * length), 4)})
        print(json.dumps({
            "kernel": lib.klt_hip_track_kernel(ctx).decode(), "shape": [W, H, N, F], "start_frame": J,
            "live_at_start": live, "order_balance": os.environ.get("KLT_ORDER_BALANCE", "1"), "waves": nin,
            "launch_us": round(length, 1), "last_entry_us": round(float((t_in[-1] - t0) * TICK_US), 1),
            "exit_us": {"p10": round(q(10), 1), "median": round(q(50), 1), "p90": round(q(90), 1),
                        "p99": round(q(99), 1), "max": round(float(end[-1]), 1)},
            "idle_share": round(idle, 4), "bound_us_per_chunk": round(idle * length, 1),
            "us_before_end_with_K_waves_left": left, "per_xcd": per_xcd}))
    for d in (dfr, dx, dy, dv, dbuf):
        lib.klt_hip_free(ctx, d)
    lib.KLTFreeTrackingContext(tc)


if __name__ == "__main__":
    main()
