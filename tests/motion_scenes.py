"""Rotating scenes that lose features in all four ways, for the tracker tests.

klt_synth_frame slides one smooth field by (-0.7, -0.3) px per frame: on it no
feature is ever lost to KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS or KLT_SMALL_DET,
none moves right or down or by more than a pixel, and the pixel values 0 and
255 never occur.  `scene` is the tests' own generator for everything else:

  * a blurred random texture (about 10 % of its pixels clip to 0 / 255) rotating
    by 1 degree and zooming by 0.6 % per frame about the image centre: motion of
    both signs in x and y, growing with the distance from the centre;
  * a flat plate sliding right by 3 px per frame: level-0 windows on it are
    flat in both frames (KLT_SMALL_DET);
  * a block whose texture slides by 6 px per frame, more than the two-level
    pyramid follows (KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS);
  * a brightness flash in frames 5 and 9.

Frames depend only on IEEE +, -, *, /, floor and rint: the rotation comes from a
literal table.  tests/golden/motion_160x120.npz records their sha256 and the
reference's tables on them (tests/golden/make_motion.py);
tests/test_motion_host.py holds the generator, the oracle and the floors below
to those records, tests/test_gpu_motion.py holds the GPU to the oracle.

The floors are conditions on the ORACLE's tables, about half of what it gives
(see FLOORS), asserted before a comparison so that a changed input cannot
quietly empty a case.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from kltabi import GOLDEN, OracleParams, OracleTracker

F32 = np.float32
SCENES = (7, 8)
W, H, NFRAMES = 160, 120, 14          # T = 13 tracked frames: chunks of 4, the last one ragged
SW, SH, SFRAMES, SFEAT = 320, 240, 11, 300   # the sharded cases
FIXTURE = GOLDEN / "motion_160x120.npz"

TRACKED, NOT_FOUND, SMALL_DET, MAX_ITERATIONS, OOB, LARGE_RESIDUE = 0, -1, -2, -3, -4, -5
LOSSES = {"OOB": OOB, "LARGE_RESIDUE": LARGE_RESIDUE, "MAX_ITERATIONS": MAX_ITERATIONS, "SMALL_DET": SMALL_DET}

# cos(t deg), sin(t deg), 1.006 ** t for t = 0..13
ROT = (
    (1.0, 0.0, 1.0),
    (0.9998476951563913, 0.01745240643728351, 1.006),
    (0.9993908270190958, 0.03489949670250097, 1.012036),
    (0.9986295347545738, 0.052335956242943835, 1.0181082160000001),
    (0.9975640502598242, 0.0697564737441253, 1.024216865296),
    (0.9961946980917455, 0.08715574274765817, 1.030362166487776),
    (0.9945218953682733, 0.10452846326765347, 1.0365443394867027),
    (0.992546151641322, 0.12186934340514748, 1.042763605523623),
    (0.9902680687415704, 0.13917310096006544, 1.0490201871567646),
    (0.9876883405951378, 0.15643446504023087, 1.0553143082797052),
    (0.984807753012208, 0.17364817766693033, 1.0616461941293835),
    (0.981627183447664, 0.1908089953765448, 1.0680160712941598),
    (0.9781476007338057, 0.20791169081775934, 1.0744241677219248),
    (0.9743700647852352, 0.224951054343865, 1.0808707127282564),
)


def texture(seed, n=256):
    a = np.random.default_rng(seed).integers(0, 256, (n, n)).astype(np.float64)

    def blur(x, k):
        for ax in (0, 1):
            x = sum(np.roll(x, s, ax) for s in range(-k, k + 1)) / (2 * k + 1)
        return x
    return np.clip((0.5 * blur(a, 1) + 0.5 * blur(a, 4) - 127.5) * 5.5 + 128, 0, 255)


def sample(T, X, Y):
    """Bilinear, float64, wrapping."""
    x0 = np.floor(X).astype(int)
    y0 = np.floor(Y).astype(int)
    ax = X - x0
    ay = Y - y0
    n = T.shape[0]
    x0 %= n
    y0 %= n
    x1 = (x0 + 1) % n
    y1 = (y0 + 1) % n
    return (1 - ax) * (1 - ay) * T[y0, x0] + ax * (1 - ay) * T[y0, x1] + (1 - ax) * ay * T[y1, x0] + ax * ay * T[y1, x1]


_scenes: dict = {}


def scene(seed, n=NFRAMES, w=W, h=H):
    """n frames [h, w] uint8 (read-only, computed once)."""
    if (seed, n, w, h) in _scenes:
        return _scenes[seed, n, w, h]
    T = texture(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    out = []
    for t in range(n):
        cs, sn, s = ROT[t]
        c, sn = cs / s, sn / s
        f = sample(T, c * (xx - cx) - sn * (yy - cy) + 128, sn * (xx - cx) + c * (yy - cy) + 128)
        x0 = 28 + 3 * t
        f[70:94, x0:x0 + 30] = 200
        f[28:52, 90:130] = sample(T, xx[28:52, 90:130] + 6 * t + 40, yy[28:52, 90:130] + 200)
        if t in (5, 9):
            f[60:96, 100:136] = np.clip(f[60:96, 100:136] * 1.5 + 30, 0, 255)
        a = np.ascontiguousarray(np.rint(f).astype(np.uint8))
        a.setflags(write=False)
        out.append(a)
    _scenes[seed, n, w, h] = out
    return out


def shard_scene(seed):
    return scene(seed, SFRAMES, SW, SH)


def placed_list():
    """251 features, val 0: a fractional lattice (221 points, x fastest), then an
    integer one (30 points: window fractions exactly 0).  Points on the plate
    see flat level-0 windows in both frames."""
    gx, gy = np.meshgrid(np.arange(26.25, 134, 6.5), np.arange(25.5, 95, 5.75))
    ix, iy = np.meshgrid(np.arange(30., 131, 20), np.arange(30., 91, 15))
    x = np.concatenate([gx.ravel(), ix.ravel()]).astype(F32)
    y = np.concatenate([gy.ravel(), iy.ravel()]).astype(F32)
    return x, y, np.zeros(len(x), np.int32)


# ---------------------------------------------------------------------------
# configurations: TrackingContext fields (klt.h) and the oracle's parameters
# ---------------------------------------------------------------------------
CONFIGS = {
    "default": {},
    "maxit3": dict(max_iterations=3),
    "lighting": dict(lighting_insensitive=1),
    "win9": dict(window_width=9, window_height=9),   # the border stays at its default 24
    "one_level": dict(search_range=2),
    "step2": dict(step_factor=2.0),
    "residue3": dict(max_residue=3.0),
}
RECORDED = ("default", "maxit3", "lighting", "win9", "one_level")  # the reference's tables in the fixture


def tc_setup(lib, name):
    """setup(t) for a klt.h tracking context record of library `lib`."""
    cfg = CONFIGS[name]

    def setup(t):
        for k, val in cfg.items():
            if k != "search_range":
                setattr(t, k, val)
        if "search_range" in cfg:
            lib.KLTChangeTCPyramid(C.byref(t), cfg["search_range"])
            lib.KLTUpdateTCBorder(C.byref(t))
    return setup


def oracle_params(oracle, name):
    cfg = CONFIGS[name]
    p = OracleParams()
    oracle.orc_default_params(C.byref(p))
    for k, val in cfg.items():
        if k != "search_range":
            setattr(p, k, val)
    if "search_range" in cfg:
        oracle.orc_change_pyramid(C.byref(p), cfg["search_range"])
        oracle.orc_update_border(C.byref(p))
    return p


_tables: dict = {}


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def oracle_table(oracle, key, frames, start, params=None):
    """The per-call loop on the oracle (sequential mode) from the list `start`:
    X, Y, V [T, n], row j = the list after frames[j + 1].  Computed once per key."""
    if key not in _tables:
        o = OracleTracker(oracle, params)
        o.params.sequentialMode = 1
        oracle.orc_set_params(o.h, C.byref(o.params))
        x, y, v = (a.copy() for a in start)
        rows = []
        for i in range(1, len(frames)):
            o.track(frames[i - 1], frames[i], x, y, v)
            rows.append((x.copy(), y.copy(), v.copy()))
        o.close()
        _tables[key] = frozen([np.stack([r[k] for r in rows]) for k in range(3)])
    return _tables[key]


def oracle_placed(oracle, seed, name="default"):
    return oracle_table(oracle, ("placed", seed, name), scene(seed), placed_list(), oracle_params(oracle, name))


def oracle_select(oracle, frame, n):
    o = OracleTracker(oracle)
    start = o.select(frame, n)
    o.close()
    return start


_starts: dict = {}


def selected_start(oracle, seed, n):
    """The oracle's selection on the scene's frame 0 (slots it cannot fill: KLT_NOT_FOUND)."""
    if (seed, n) not in _starts:
        _starts[seed, n] = frozen(list(oracle_select(oracle, scene(seed)[0], n)))
    return _starts[seed, n]


def oracle_shard(oracle, seed):
    """The 320x240 scene from 300 selected features: the start list and the table [10, 300]."""
    fr = shard_scene(seed)
    if ("shard", seed) not in _starts:
        _starts["shard", seed] = frozen(list(oracle_select(oracle, fr[0], SFEAT)))
    start = _starts["shard", seed]
    return start, oracle_table(oracle, ("shard", seed), fr, start)


def klt_table(lib, frames, start, setup=None, sequential=True):
    """The same loop through klt.h (KLTTrackFeatures per frame) on library `lib`."""
    from kltabi import arrays_to_fl, fl_to_arrays, u8ptr
    h, w = frames[0].shape
    tc = lib.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1 if sequential else 0
    tc.contents.writeInternalImages = 0
    tc.contents.affineConsistencyCheck = -1
    if setup:
        setup(tc.contents)
    fl = lib.KLTCreateFeatureList(len(start[0]))
    arrays_to_fl(fl, *start)
    rows = []
    for i in range(1, len(frames)):
        lib.KLTTrackFeatures(tc, u8ptr(frames[i - 1]), u8ptr(frames[i]), w, h, fl)
        rows.append(fl_to_arrays(fl))
    lib.KLTFreeFeatureList(fl)
    lib.KLTFreeTrackingContext(tc)
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


# ---------------------------------------------------------------------------
# what a table holds
# ---------------------------------------------------------------------------
def first_losses(V, start_v=None):
    """Per feature (row, status) of its first loss in V [T, n]; row -1: the
    start list's own status (a slot the selection did not fill)."""
    out = []
    for k in range(V.shape[1]):
        if start_v is not None and start_v[k] < 0:
            out.append((-1, int(start_v[k])))
            continue
        lost = np.nonzero(V[:, k] < 0)[0]
        if len(lost):
            out.append((int(lost[0]), int(V[lost[0], k])))
    return out


def status_counts(V, start_v=None):
    """First loss per feature by status name, the slots never filled, and the
    features alive after the last row."""
    fl = first_losses(V, start_v)
    c = {name: sum(1 for _, s in fl if s == code) for name, code in LOSSES.items()}
    c["NOT_FOUND"] = sum(1 for _, s in fl if s == NOT_FOUND)
    c["other"] = len(fl) - sum(c.values())
    c["alive"] = V.shape[1] - len(fl)
    return c


def frame1_motion(table, start):
    """dx, dy of the features tracked in the first frame."""
    X, Y, V = table
    ok = (V[0] >= 0) & (start[2] >= 0)
    return (X[0] - start[0])[ok], (Y[0] - start[1])[ok]


def band_changes(table, start, h, world):
    """Tracked features whose owner band (edges at h * r // world, by y) changes
    between consecutive lists: (downward, upward)."""
    edges = np.array([h * r // world for r in range(1, world)], np.float32)
    ys = np.concatenate([start[1][None], table[1]])
    vs = np.concatenate([start[2][None], table[2]])
    down = up = 0
    for j in range(1, len(ys)):
        ok = (vs[j - 1] >= 0) & (vs[j] >= 0)
        a = np.searchsorted(edges, ys[j - 1][ok], side="right")
        b = np.searchsorted(edges, ys[j][ok], side="right")
        down += int((b > a).sum())
        up += int((b < a).sum())
    return down, up


# ---------------------------------------------------------------------------
# floors: about half the smaller value the oracle gives on scenes 7 / 8
# ---------------------------------------------------------------------------
# placed, default           OOB 41/35  LARGE_RESIDUE 125/128  MAX_ITERATIONS 5/4      SMALL_DET 7/6  alive 73/78
# placed, max_iterations 3  OOB 22/18  LARGE_RESIDUE 61/74    MAX_ITERATIONS 118/116  SMALL_DET 7/6  alive 43/37
# placed, lighting          OOB 21/25  LARGE_RESIDUE 140/140  MAX_ITERATIONS 5/6      SMALL_DET 8/6  alive 77/74
# placed, 9x9               OOB 30/30  LARGE_RESIDUE 138/135  MAX_ITERATIONS 4/6      SMALL_DET 4/2  alive 75/78
# placed, one level         OOB 0/0    LARGE_RESIDUE 142/146  MAX_ITERATIONS 6/2      SMALL_DET 6/6  alive 97/97
FLOORS = {
    "default": dict(LARGE_RESIDUE=60, OOB=15, MAX_ITERATIONS=2, SMALL_DET=3, alive=35),
    "maxit3": dict(MAX_ITERATIONS=55),
    "lighting": dict(LARGE_RESIDUE=60, SMALL_DET=1, MAX_ITERATIONS=2),
    "win9": dict(LARGE_RESIDUE=60, SMALL_DET=1, MAX_ITERATIONS=2),
    "one_level": dict(LARGE_RESIDUE=70, SMALL_DET=3, MAX_ITERATIONS=1),
}
REPLACE_FLOORS = {1: dict(total=100, each=0), 3: dict(total=50, each=5)}   # refilled slots
SHARD_FLOORS = {3: (5, 8), 4: (9, 11)}                                     # band changes (downward, upward)


def check_placed(name, table, start=None):
    """The floors of a placed-list case on the oracle's table."""
    start = placed_list() if start is None else start
    c = status_counts(table[2])
    if name in FLOORS:
        for what, least in FLOORS[name].items():
            assert c[what] >= least, (name, what, c)
    else:  # step2, residue3: not measured in advance
        assert sum(1 for s in LOSSES if c[s] > 0) >= 2 and c["alive"] >= 10, (name, c)
    if name == "default":
        chunks = {row // 4 for row, _ in first_losses(table[2])}
        assert len(chunks) >= 3, chunks
        dx, dy = frame1_motion(table, start)
        assert dx.min() < 0 < dx.max() and dy.min() < 0 < dy.max(), (dx.min(), dx.max(), dy.min(), dy.max())
        assert np.abs(dx).max() >= 3
    return c


def check_replace(every, points):
    """points: test_gpu_replace.oracle_loop's (frame, lost, filled) per replacing frame."""
    fl = REPLACE_FLOORS[every]
    filled = [p[2] for p in points]
    assert len(filled) == (NFRAMES - 1) // every
    assert sum(filled) >= fl["total"] and min(filled) >= fl["each"], filled
    return filled


def check_shard(world, table, start):
    down, up = band_changes(table, start, SH, world)
    assert down >= SHARD_FLOORS[world][0] and up >= SHARD_FLOORS[world][1], (world, down, up)
    return down, up
