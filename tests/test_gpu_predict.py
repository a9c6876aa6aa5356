"""The motion prior on the GPU (klt_hip_set_predict, klt_amd_set_prediction)
against its CPU statement (tests/native/predict_oracle.c through
predict_scenes.shim_table): x, y, val and the state (vx, vy), bit for bit, on
every call that honours the setting, and every call that refuses it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import predict_scenes as ps
from kltabi import OracleParams, arrays_to_fl, fl_to_arrays, u8ptr
from motion_scenes import F32
from test_predict_host import assert_scene_conditions, bits, first_frame, replace_case, seeded

pytestmark = pytest.mark.gpu

T, W, H = ps.T, ps.W, ps.H


def assert_rows_equal(got, want, rows=None, names="x y val vx vy"):
    """[T, n] tables, bit patterns."""
    for g, w, name in zip(got, want, names.split()):
        g, w = (g, w) if rows is None else (g[rows], w[rows])
        assert g.shape == w.shape, name
        bad = np.argwhere(bits(g) != bits(w))
        assert not len(bad), f"{name} differs first at (frame, feature) {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


class Dev:
    """One device context with the scene's frames, a list and its state in
    device memory, and tables of all five arrays."""

    def __init__(self, gpu, frames, start, state=None, predict=True, setup=None):
        from kltamd.device import H2D, PyrDesc, TrackDesc, check
        self.gpu, self.check = gpu, check
        self.n = n = len(start[0])
        self.tc = tc = gpu.KLTCreateTrackingContext()
        tc.contents.sequentialMode = 1
        if setup:
            setup(tc.contents)
        self.ctx = ctx = gpu.klt_amd_device_context(tc)
        stack = np.ascontiguousarray(np.stack(frames))
        self.nbuf = []
        self.dfr = self.malloc(stack.nbytes)
        self.put(self.dfr, stack)
        vx, vy = (np.zeros(n, F32), np.zeros(n, F32)) if state is None else state
        self.list = [self.malloc(4 * n) for _ in range(5)]       # x, y, val, vx, vy
        for d, a in zip(self.list, (*start, vx, vy)):
            self.put(d, np.ascontiguousarray(a))
        self.tabs = [self.malloc(4 * n * T) for _ in range(5)]
        for d in self.tabs:                                           # every cell must be written
            self.put(d, np.full((T, n), 7.0, F32))
        self.pd, self.td = PyrDesc(), TrackDesc()
        gpu.klt_amd_pyr_desc(tc, W, H, tc.contents.nPyramidLevels, 1, C.byref(self.pd))
        gpu.klt_amd_track_desc(tc, C.byref(self.td))
        if predict:
            self.predict(1)

    def malloc(self, nbytes):
        d = self.gpu.klt_hip_malloc(self.ctx, nbytes)
        assert d
        self.nbuf.append(d)
        return d

    def put(self, d, a):
        from kltamd.device import H2D
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_memcpy(self.ctx, d, a.ctypes.data, a.nbytes, H2D), "h2d")

    def get(self, d, shape, dtype):
        from kltamd.device import D2H
        a = np.empty(shape, dtype)
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_sync(self.ctx), "sync")
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_memcpy(self.ctx, a.ctypes.data, d, a.nbytes, D2H), "d2h")
        return a

    def predict(self, on, row=0):
        g, n = self.gpu, self.n
        assert g.klt_hip_set_predict(self.ctx, on, self.list[3] if on else None, self.list[4] if on else None) == 0
        assert g.klt_hip_set_predict_table(self.ctx, self.tabs[3] + 4 * n * row if on else None,
                                           self.tabs[4] + 4 * n * row if on else None, n) == 0

    def frame(self, i):
        return self.dfr + i * W * H

    def begin(self, i=0):
        self.check(self.gpu, self.ctx, self.gpu.klt_hip_frames_begin(self.ctx, C.byref(self.pd), self.frame(i), W), "begin")

    def track_frames(self, j0, nf, chunk, tables=True):
        """frames j0 + 1 .. j0 + nf; their rows j0 .."""
        n, off = self.n, 4 * self.n * j0
        on = C.c_int()
        assert self.gpu.klt_hip_get_predict(self.ctx, C.byref(on), None, None) == 0
        if on.value and tables:  # the state's rows beside the list's
            self.predict(1, j0)
        tx, ty, tv = (t + off if tables else None for t in self.tabs[:3])
        return self.gpu.klt_hip_track_frames(self.ctx, C.byref(self.pd), C.byref(self.td), self.frame(1 + j0), W, W * H,
                                             nf, chunk, *self.list[:3], n, tx, ty, tv, n)

    def lists(self):
        n = self.n
        return tuple(self.get(d, n, np.int32 if k == 2 else F32) for k, d in enumerate(self.list))

    def tables(self):
        n = self.n
        return tuple(self.get(d, (T, n), np.int32 if k == 2 else F32) for k, d in enumerate(self.tabs))

    def list_bytes(self):
        return b"".join(a.tobytes() for a in self.lists())

    def error(self):
        m = self.gpu.klt_hip_last_error(self.ctx)
        return m.decode() if m else ""

    def close(self):
        self.gpu.klt_hip_sync(self.ctx)
        self.predict(0)
        for d in self.nbuf:
            self.gpu.klt_hip_free(self.ctx, d)
        self.gpu.KLTFreeTrackingContext(self.tc)


@pytest.fixture
def dev(gpu):
    made = []

    def make(frames, start, **kw):
        made.append(Dev(gpu, frames, start, **kw))
        return made[-1]
    yield make
    for d in made:
        d.close()


def want_lattice(seed):
    assert_scene_conditions(seed)  # before any comparison
    return ps.shim_lattice(seed)[:5]


# ---------------------------------------------------------------------------
# the calls that honour the setting
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ps.SEEDS)
def test_per_call_track_loop(gpu, dev, seed):
    want = want_lattice(seed)
    d = dev(ps.scene(seed), ps.lattice())
    g, rows = d.gpu, []
    d.check(g, d.ctx, g.klt_hip_build_pyramid(d.ctx, 0, C.byref(d.pd), d.frame(0), W, 0), "pyramid")
    for i in range(1, T + 1):
        s1, s2 = (i - 1) % 2, i % 2
        d.check(g, d.ctx, g.klt_hip_build_pyramid(d.ctx, s2, C.byref(d.pd), d.frame(i), W, 0), "pyramid")
        d.predict(1, i - 1)  # a call writes row 0 of the table it is given
        d.check(g, d.ctx, g.klt_hip_track(d.ctx, s1, s2, C.byref(d.td), *d.list[:3], d.n, 1), "track")
        assert g.klt_hip_track_kernel(d.ctx) == b"kltdev::k_track7_pred<true, 2>"
        rows.append(d.lists())
    got = tuple(np.stack([r[k] for r in rows]) for k in range(5))
    assert_rows_equal(got, want)
    tabs = d.tables()
    assert_rows_equal(tabs[3:], want[3:], names="vx vy")


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_track_sequence_steps(gpu, dev, seed):
    want = want_lattice(seed)
    d = dev(ps.scene(seed), ps.lattice())
    g = d.gpu
    d.check(g, d.ctx, g.klt_hip_build_pyramid(d.ctx, 0, C.byref(d.pd), d.frame(0), W, 0), "pyramid")
    cur = C.c_int(0)
    d.check(g, d.ctx, g.klt_hip_track_sequence(d.ctx, C.byref(d.pd), C.byref(d.td), d.dfr, W, W * H, 1, T, *d.list[:3],
                                               d.n, C.byref(cur)), "track_sequence")
    assert_rows_equal(d.lists(), tuple(w[-1] for w in want))


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("chunk", [1, 4, 13])
def test_track_frames_chunks(gpu, dev, seed, chunk):
    """Chunks of 4: the last one is ragged."""
    want = want_lattice(seed)
    d = dev(ps.scene(seed), ps.lattice())
    d.begin()
    d.check(d.gpu, d.ctx, d.track_frames(0, T, chunk), "frames")
    assert d.gpu.klt_hip_track_kernel(d.ctx) == b"kltdev::k_track7_pred<true, 2>"
    assert_rows_equal(d.tables(), want)
    assert_rows_equal(d.lists(), tuple(w[-1] for w in want))


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_one_call_equals_two(gpu, dev, seed):
    """13 frames == 6 + 7 frames: the state is carried through the arrays."""
    want = want_lattice(seed)
    d = dev(ps.scene(seed), ps.lattice())
    d.begin()
    d.check(d.gpu, d.ctx, d.track_frames(0, 6, 4), "frames")
    mid = d.lists()
    assert_rows_equal(mid, tuple(w[5] for w in want))
    assert mid[3].any()
    d.check(d.gpu, d.ctx, d.track_frames(6, 7, 4), "frames")
    assert_rows_equal(d.tables(), want)
    assert_rows_equal(d.lists(), tuple(w[-1] for w in want))


_ROWS = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                    C.POINTER(C.c_int), C.c_long)


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("host_state", [True, False])
def test_track_frames_host(gpu, dev, seed, host_state):
    """The state goes up before the first launch and comes back with the list:
    from host arrays as x, y and val are, or from device arrays."""
    want = want_lattice(seed)
    frames = [np.ascontiguousarray(f) for f in ps.scene(seed)]
    d = dev(frames, ps.lattice(), predict=False)
    n = d.n
    x, y, v = (a.copy() for a in ps.lattice())
    vx, vy = np.zeros(n, F32), np.zeros(n, F32)
    if host_state:
        assert gpu.klt_hip_set_predict(d.ctx, 1, vx.ctypes.data, vy.ctypes.data) == 0
    else:
        d.predict(1)
        assert gpu.klt_hip_set_predict_table(d.ctx, None, None, 0) == 0
    X, Y, V = np.zeros((T, n), F32), np.zeros((T, n), F32), np.zeros((T, n), np.int32)

    def rows(user, frame0, nframes, f0, f1, rx, ry, rv, stride):
        for j in range(nframes):
            for dst, src in ((X, rx), (Y, ry), (V, rv)):
                dst[frame0 + j, f0:f1] = np.ctypeslib.as_array(src, shape=((j + 1) * stride,))[j * stride + f0:j * stride + f1]

    cb = _ROWS(rows)
    arr = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    rc = gpu.klt_hip_track_frames_host(d.ctx, C.byref(d.pd), C.byref(d.td), arr, len(frames), 1, 4, x.ctypes.data,
                                       y.ctypes.data, v.ctypes.data, n, cb, None)
    d.check(gpu, d.ctx, rc, "frames_host")
    if not host_state:
        vx, vy = d.lists()[3:]
    # the setting still names the caller's arrays
    on, px, py = C.c_int(), C.c_void_p(), C.c_void_p()
    assert gpu.klt_hip_get_predict(d.ctx, C.byref(on), C.byref(px), C.byref(py)) == 0
    assert on.value == 1 and px.value == (vx.ctypes.data if host_state else d.list[3])
    assert gpu.klt_hip_set_predict(d.ctx, 0, None, None) == 0
    assert_rows_equal((X, Y, V), want[:3])
    assert_rows_equal((x, y, v, vx, vy), tuple(w[-1] for w in want))


# ---------------------------------------------------------------------------
# the klt.h surface
# ---------------------------------------------------------------------------
def klt_context(gpu, start):
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    fl = gpu.KLTCreateFeatureList(len(start[0]))
    arrays_to_fl(fl, *start)
    return tc, fl


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_klt_track_sequence(gpu, seed):
    want = want_lattice(seed)
    frames = [np.ascontiguousarray(f) for f in ps.scene(seed)]
    tc, fl = klt_context(gpu, ps.lattice())
    assert gpu.klt_amd_set_prediction(tc, 1) == 0
    n = fl.contents.nFeatures
    ft = gpu.KLTCreateFeatureTable(T, n)
    arr = (C.POINTER(C.c_ubyte) * len(frames))(*[u8ptr(f) for f in frames])
    # two calls: the state is kept in the tracking context between them
    gpu.KLTTrackSequence(tc, arr, 7, W, H, fl, ft, 0)
    arr2 = (C.POINTER(C.c_ubyte) * 8)(*[u8ptr(f) for f in frames[6:]])
    gpu.KLTTrackSequence(tc, arr2, 8, W, H, fl, ft, 6)
    X = np.array([[ft.contents.feature[k][j].contents.x for k in range(n)] for j in range(T)], F32)
    Y = np.array([[ft.contents.feature[k][j].contents.y for k in range(n)] for j in range(T)], F32)
    V = np.array([[ft.contents.feature[k][j].contents.val for k in range(n)] for j in range(T)], np.int32)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    assert_rows_equal((X, Y, V), want[:3])


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_klt_track_features_loop(gpu, seed):
    """A list keeps a lost feature's last position (the reference leaves the
    slot untouched), so x and y are compared where the feature is tracked."""
    want = want_lattice(seed)
    frames = [np.ascontiguousarray(f) for f in ps.scene(seed)]
    tc, fl = klt_context(gpu, ps.lattice())
    assert gpu.klt_amd_set_prediction(tc, 1) == 0
    for i in range(1, T + 1):
        gpu.KLTTrackFeatures(tc, u8ptr(frames[i - 1]), u8ptr(frames[i]), W, H, fl)
        x, y, v = fl_to_arrays(fl)
        ok = v == 0
        assert np.array_equal(v, want[2][i - 1]), i
        assert np.array_equal(bits(x[ok]), bits(want[0][i - 1][ok])) and np.array_equal(bits(y[ok]), bits(want[1][i - 1][ok])), i
    # turned off and on again: the state is zero, the next frame the plain tracker's
    assert gpu.klt_amd_set_prediction(tc, 0) == 0
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)


def test_klt_prediction_refuses_fb(gpu):
    """A KLTError ends the process: run in a child."""
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = %r; import numpy as np, ctypes as C, kltamd\n"
            "g = kltamd.load(); g.KLTSetVerbosity(0)\n"
            "tc = g.KLTCreateTrackingContext(); fl = g.KLTCreateFeatureList(4)\n"
            "assert g.klt_amd_set_prediction(tc, 1) == 0 and g.klt_amd_set_fb_check(tc, 1, 1.0) == 0\n"
            "a = np.zeros((64, 64), np.uint8); p = a.ctypes.data_as(C.POINTER(C.c_ubyte))\n"
            "g.KLTTrackFeatures(tc, p, p, 64, 64, fl)\nprint('survived')\n") % [str(ps.SHIM_LIB.parents[3])]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "motion prior does not combine with the forward-backward check" in r.stderr


# ---------------------------------------------------------------------------
# rule 3, rule 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("big", [1e4, np.inf])
def test_huge_state_is_the_plain_tracker(gpu, dev, seed, big):
    """Every third feature seeded with (big, -big): its start's window is
    outside the coarsest level, so frame 1 is the plain tracker's."""
    state = seeded(big, -big)
    want = first_frame(seed, state)
    plain = first_frame(seed, None, predict=False)
    for k in range(3):
        assert np.array_equal(bits(want[k]), bits(plain[k]))  # on the CPU first
    fr = ps.scene(seed)[:2]
    d = dev(fr, ps.lattice(), state=state)
    d.begin()
    d.check(d.gpu, d.ctx, d.track_frames(0, 1, 1, tables=False), "frames")
    got = d.lists()
    assert_rows_equal(got, tuple(w[0] for w in want[:5]))
    # ... and what the tracker gives with the setting off
    p = dev(fr, ps.lattice(), predict=False)
    p.begin()
    p.check(p.gpu, p.ctx, p.track_frames(0, 1, 1, tables=False), "frames")
    assert_rows_equal(p.lists()[:3], got[:3], rows=np.arange(0, d.n, 3))
    assert_rows_equal(p.lists()[:3], got[:3])


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("chunk", [4, 13])
def test_replacement_inside_the_call(gpu, dev, seed, chunk):
    """klt_hip_set_frames_replace every 3 frames against the shim + orc_replace
    loop, from orc_select's list (val > 0: rule 1); a replaced slot comes back
    with val > 0 and a zero state."""
    from kltamd.device import ReplaceDesc
    start, want = replace_case(seed)
    V = want[2]
    assert (start[2] > 0).all()
    assert sum(int(((V[j] > 0) & (V[j + 1] == 0)).sum()) for j in (2, 5, 8)) >= 1  # on the oracle first
    d = dev(ps.scene(seed), start)
    rd = ReplaceDesc.from_tc(d.tc.contents, 3)
    assert gpu.klt_hip_set_frames_replace(d.ctx, C.byref(rd)) == 0
    d.begin()
    rc = d.track_frames(0, T, chunk)
    assert gpu.klt_hip_set_frames_replace(d.ctx, None) == 0
    d.check(gpu, d.ctx, rc, "frames")
    assert_rows_equal(d.tables(), want[:5])
    assert_rows_equal(d.lists(), tuple(w[-1] for w in want[:5]))


# ---------------------------------------------------------------------------
# off: the kernels of before; refusals
# ---------------------------------------------------------------------------
def test_setting_off_keeps_the_kernel(gpu, dev):
    fr = ps.scene(7)[:3]
    d = dev(fr, ps.lattice(), predict=False)
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, 2, 2), "frames")
    assert gpu.klt_hip_track_kernel(d.ctx) == b"kltdev::k_track7<false, true, 2, false, true>"  # lazy gradients
    d.predict(1)
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, 2, 2), "frames")
    assert gpu.klt_hip_track_kernel(d.ctx) == b"kltdev::k_track7_pred<true, 2>"
    d.predict(0)
    d.begin()
    d.check(gpu, d.ctx, d.track_frames(0, 2, 2), "frames")
    assert gpu.klt_hip_track_kernel(d.ctx) == b"kltdev::k_track7<false, true, 2, false, true>"
    assert gpu.klt_hip_ctx_reset(d.ctx) == 0  # ... and a reset turns it off
    on = C.c_int(1)
    assert gpu.klt_hip_get_predict(d.ctx, C.byref(on), None, None) == 0 and on.value == 0


def test_refusals(gpu, dev):
    """-1 and a message naming the setting, before any launch: x, y, val and
    the state byte for byte as they were."""
    from kltamd.device import FAST, AffineDesc, ReplaceDesc, TrackDesc
    fr = ps.scene(7)[:4]
    state = seeded(1.5, -0.5)
    d = dev(fr, ps.lattice(), state=state)
    g, ctx, n = gpu, d.ctx, d.n
    d.begin()
    before = d.list_bytes()
    x, y, v = d.list[:3]

    def td(**kw):
        t = TrackDesc.from_buffer_copy(d.td)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    def frames(t=None):
        t = t or d.td
        return g.klt_hip_track_frames(ctx, C.byref(d.pd), C.byref(t), d.frame(1), W, W * H, 3, 2, x, y, v, n, None, None,
                                      None, 0)

    def refused(rc, what):
        assert rc == -1, what
        assert "klt_hip_set_predict" in d.error(), (what, d.error())
        assert d.list_bytes() == before, what

    # the forward-backward check, the affine check, fast sums
    assert g.klt_hip_set_fb(ctx, 1, 1.0) == 0
    refused(frames(), "fb")
    assert g.klt_hip_set_fb(ctx, 0, 0.0) == 0
    ad = AffineDesc(0, 15, 15, 10, 0.01, 0.1, 0.02, 10.0, 1.5, 1.0, 0)
    scratch = d.malloc(4 * 6 * n)
    assert g.klt_hip_set_frames_affine(ctx, C.byref(ad), scratch, scratch) == 0
    refused(frames(), "affine inside the launch")
    assert g.klt_hip_set_frames_affine(ctx, None, None, None) == 0
    refused(frames(td(reduction=FAST)), "fast sums")
    # the generic tracker: other windows, lighting-insensitive mode, forced
    refused(frames(td(window_width=9, window_height=9)), "window 9")
    refused(frames(td(lighting_insensitive=1)), "lighting-insensitive")
    assert g.klt_hip_set_track_impl(ctx, 1) == 0
    refused(frames(), "generic kernel")
    assert g.klt_hip_set_track_impl(ctx, 0) == 0
    # band calls and the sharded driver
    esc = d.malloc(4)
    refused(g.klt_hip_track_frames_band(ctx, C.byref(d.pd), C.byref(d.td), d.frame(1), W, W * H, 2, x, y, v, n, 0.0,
                                        float(H), 0, H, esc, None, 0), "band")
    s = g.klt_shard_create_local(ctx, 0, 1, H, 16)
    assert s, g.klt_shard_create_error()
    rc = g.klt_shard_track(s, C.byref(d.pd), C.byref(d.td), d.frame(1), W, W * H, 2, None, 0, x, y, v, n, None, None)
    msg = g.klt_shard_last_error(s).decode()
    g.klt_shard_destroy(s)
    assert rc < 0 and "klt_hip_set_predict" in msg and d.list_bytes() == before
    # the multi-sequence calls
    counts = (C.c_int * 1)(n)
    refused(g.klt_hip_multi_covers(ctx, C.byref(d.pd), C.byref(d.td)), "multi_covers")
    refused(g.klt_hip_track_frames_multi(ctx, C.byref(d.pd), C.byref(d.td), d.dfr, W, W * H, W * H, 1, 2, 2, counts, x, y,
                                         v, None, None, None, 0), "multi")
    rd = ReplaceDesc.from_tc(d.tc.contents, 2)
    refused(g.klt_hip_track_frames_multi_replace(ctx, C.byref(d.pd), C.byref(d.td), C.byref(rd), 0, d.dfr, W, W * H,
                                                 W * H, 1, 2, 2, counts, x, y, v, None, None, None, 0, None, None, None),
            "multi_replace")
    # klt_hip_track with host arrays, klt_hip_track_affine
    for slot in (0, 1):
        d.check(g, ctx, g.klt_hip_build_pyramid(ctx, slot, C.byref(d.pd), d.frame(slot), W, 0), "pyramid")
    hx, hy, hv = (a.copy() for a in ps.lattice())
    hb = hx.tobytes() + hy.tobytes() + hv.tobytes()
    refused(g.klt_hip_track(ctx, 0, 1, C.byref(d.td), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data, n, 0), "host arrays")
    assert hx.tobytes() + hy.tobytes() + hv.tobytes() == hb
    aff, st = np.zeros((n, 6), F32), np.zeros(n, np.int32)
    assert g.klt_hip_affine_reserve(ctx, n, 15, 15) >= 0
    fn = g.klt_hip_track_affine  # another module may have bound its own pointer types: cast to whatever they are
    ptrs = [C.cast(p, t) for p, t in zip((C.pointer(d.td), C.pointer(ad), hx.ctypes.data, hy.ctypes.data, hv.ctypes.data,
                                          aff.ctypes.data, st.ctypes.data), fn.argtypes[3:10])]
    refused(fn(ctx, 0, 1, *ptrs, n), "track_affine")
    assert hx.tobytes() + hy.tobytes() + hv.tobytes() == hb
    # a table whose rows are too short
    assert g.klt_hip_set_predict_table(ctx, d.tabs[3], d.tabs[4], n - 1) == 0
    rc = frames()
    assert rc == -1 and "table stride" in d.error() and d.list_bytes() == before
    # the setting is still on, with the caller's arrays; the call it covers runs
    on, px, py = C.c_int(), C.c_void_p(), C.c_void_p()
    assert g.klt_hip_get_predict(ctx, C.byref(on), C.byref(px), C.byref(py)) == 0
    assert (on.value, px.value, py.value) == (1, d.list[3], d.list[4])
    assert g.klt_hip_set_predict_table(ctx, None, None, 0) == 0
    d.check(g, ctx, frames(), "frames")
    want = ps.shim_table(("refusals", 7), fr, ps.lattice(), state=state)
    assert_rows_equal(d.lists(), tuple(w[-1] for w in want[:5]))
