"""The region mask through the klt.h layer (klt_amd_set_mask, include/klt_amd.h)
against its CPU statement (tests/native/mask_oracle.c), on the inputs of
test_gpu_mask_select.py and test_gpu_mask_track.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import mask_scenes as ms
from kltabi import arrays_to_fl, fl_to_arrays, load_dataset, u8ptr
from motion_scenes import F32, H, W, placed_list, scene
from test_mask_host import bits, img0_mask, same

pytestmark = pytest.mark.gpu

T = ms.T
BOTH = ms.MASK_SELECT | ms.MASK_TRACK


def context(gpu, start=None, n=None, sequential=1):
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = sequential
    fl = gpu.KLTCreateFeatureList(len(start[0]) if start is not None else n)
    if start is not None:
        arrays_to_fl(fl, *start)
    return tc, fl


def set_mask(gpu, tc, mask, flags):
    if mask is None:
        return gpu.klt_amd_set_mask(tc, None, 0, 0, 0)
    assert mask.flags.c_contiguous and mask.shape[1] == mask.strides[0]
    return gpu.klt_amd_set_mask(tc, mask.ctypes.data, mask.shape[1], mask.shape[0], flags)


def table_of(ft, n, rows):
    X = np.array([[ft.contents.feature[k][j].contents.x for k in range(n)] for j in range(rows)], F32)
    Y = np.array([[ft.contents.feature[k][j].contents.y for k in range(n)] for j in range(rows)], F32)
    V = np.array([[ft.contents.feature[k][j].contents.val for k in range(n)] for j in range(rows)], np.int32)
    return X, Y, V


def frame_array(frames):
    return (C.POINTER(C.c_ubyte) * len(frames))(*[u8ptr(f) for f in frames])


def test_select_and_replace(gpu):
    """KLTSelectGoodFeatures and KLTReplaceLostFeatures (no kept pyramid) on img0 with 150 features."""
    img = load_dataset(n=1)[0]
    h, w = img.shape
    mask, plain = img0_mask(img)
    s = ms.Shim(sequential=0)
    sel = s.select_mask(img, 150, mask)
    rep = tuple(a.copy() for a in sel)
    rep[2][::3] = -3
    lost = tuple(a.copy() for a in rep)
    s.replace_mask(img, *rep, mask)
    s.close()
    assert ((rep[2] > 0) & (lost[2] < 0)).sum() >= 10
    tc, fl = context(gpu, n=150, sequential=0)
    assert set_mask(gpu, tc, np.array(mask), ms.MASK_SELECT) == 0
    gpu.KLTSelectGoodFeatures(tc, u8ptr(img), w, h, fl)
    assert same(fl_to_arrays(fl), sel)
    arrays_to_fl(fl, *lost)
    gpu.KLTReplaceLostFeatures(tc, u8ptr(img), w, h, fl)
    assert same(fl_to_arrays(fl), rep)
    # bad flags: -1, the mask stays; NULL clears it
    assert gpu.klt_amd_set_mask(tc, mask.ctypes.data, w, h, 4) == -1
    gpu.KLTSelectGoodFeatures(tc, u8ptr(img), w, h, fl)
    assert same(fl_to_arrays(fl), sel)
    assert set_mask(gpu, tc, None, 0) == 0
    gpu.KLTSelectGoodFeatures(tc, u8ptr(img), w, h, fl)
    assert same(fl_to_arrays(fl), plain)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)


@pytest.mark.parametrize("seed", ms.SEEDS)
def test_track_features_loop(gpu, seed):
    """A list keeps a lost feature's last position (the reference leaves the
    slot untouched), so x and y are compared where the feature is tracked."""
    ms.assert_scene_conditions(seed)
    want = ms.placed_table(seed)
    frames = [np.ascontiguousarray(f) for f in scene(seed)]
    tc, fl = context(gpu, placed_list())
    assert set_mask(gpu, tc, ms.scene_mask(), ms.MASK_TRACK) == 0
    for i in range(1, T + 1):
        gpu.KLTTrackFeatures(tc, u8ptr(frames[i - 1]), u8ptr(frames[i]), W, H, fl)
        x, y, v = fl_to_arrays(fl)
        ok = v == 0
        assert np.array_equal(v, want[2][i - 1]), i
        assert np.array_equal(bits(x[ok]), bits(want[0][i - 1][ok])) and np.array_equal(bits(y[ok]), bits(want[1][i - 1][ok])), i
    assert (v == ms.MASKED).sum() >= ms.FLOORS["masked"]
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)


@pytest.mark.parametrize("seed", ms.SEEDS)
@pytest.mark.parametrize("every", [0, 3])
def test_track_sequence(gpu, seed, every):
    """KLTTrackSequence (tracking use) and KLTTrackSequenceReplace (both uses), in two calls."""
    ms.assert_scene_conditions(seed)
    mask = ms.scene_mask()
    want = ms.placed_table(seed) if not every else \
        ms.shim_table(("replace", seed), scene(seed), placed_list(), track_mask=mask, select_mask=mask, every=3)
    frames = [np.ascontiguousarray(f) for f in scene(seed)]
    tc, fl = context(gpu, placed_list())
    assert set_mask(gpu, tc, mask, BOTH if every else ms.MASK_TRACK) == 0
    n = fl.contents.nFeatures
    ft = gpu.KLTCreateFeatureTable(T, n)
    if every:
        gpu.KLTTrackSequenceReplace(tc, frame_array(frames[:7]), 7, W, H, fl, ft, 0, every)
        gpu.KLTTrackSequenceReplace(tc, frame_array(frames[6:]), 8, W, H, fl, ft, 6, every)
    else:
        gpu.KLTTrackSequence(tc, frame_array(frames[:7]), 7, W, H, fl, ft, 0)
        gpu.KLTTrackSequence(tc, frame_array(frames[6:]), 8, W, H, fl, ft, 6)
    got = table_of(ft, n, T)
    gpu.KLTFreeFeatureTable(ft)
    gpu.KLTFreeFeatureList(fl)
    gpu.KLTFreeTrackingContext(tc)
    for g, w, name in zip(got, want[:3], "x y val".split()):
        bad = np.argwhere(bits(g) != bits(w))
        assert not len(bad), f"{name} differs first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"
    assert (got[2] == ms.MASKED).sum() >= ms.FLOORS["masked"]


@pytest.mark.parametrize("flags", [ms.MASK_SELECT, BOTH])
def test_track_sequences_replace(gpu, flags):
    """Scenes 7 and 8 in one KLTTrackSequencesReplace: with the selection use
    alone on the multi-sequence call, with both uses on its per-sequence loop."""
    mask = ms.scene_mask()
    tm = mask if flags & ms.MASK_TRACK else None
    wants = [ms.shim_table(("seqs", s, flags), scene(s), placed_list(), track_mask=tm, select_mask=mask, every=3)
             for s in ms.SEEDS]
    tc = gpu.KLTCreateTrackingContext()
    tc.contents.sequentialMode = 1
    assert set_mask(gpu, tc, mask, flags) == 0
    n = len(placed_list()[0])
    fls, fts, keep = [], [], []
    for s in ms.SEEDS:
        fl = gpu.KLTCreateFeatureList(n)
        arrays_to_fl(fl, *placed_list())
        fls.append(fl)
        fts.append(gpu.KLTCreateFeatureTable(T, n))
        frames = [np.ascontiguousarray(f) for f in scene(s)]
        keep.append(frames)
    from kltamd.abi import FL, FT
    U8P = C.POINTER(C.c_ubyte)
    arrs = [frame_array(f) for f in keep]
    seqs = (C.POINTER(U8P) * 2)(*[C.cast(a, C.POINTER(U8P)) for a in arrs])
    gpu.KLTTrackSequencesReplace(tc, seqs, 2, T + 1, W, H, (FL * 2)(*fls), (FT * 2)(*fts), 0, 3)
    ctx = gpu.klt_amd_device_context(tc)
    if flags == ms.MASK_SELECT:  # the multi-sequence call ran
        assert gpu.klt_hip_track_kernel(ctx) == b"kltdev::k_track7_multi<2>"
    for k, s in enumerate(ms.SEEDS):
        got = table_of(fts[k], n, T)
        want = wants[k]
        assert np.array_equal(got[2], want[2]), s
        live = got[2] >= 0
        assert np.array_equal(bits(got[0][live]), bits(want[0][live])), s
        assert np.array_equal(bits(got[1][live]), bits(want[1][live])), s
        if flags & ms.MASK_TRACK:
            assert (got[2] == ms.MASKED).sum() >= ms.FLOORS["masked"]
        gpu.KLTFreeFeatureTable(fts[k])
        gpu.KLTFreeFeatureList(fls[k])
    gpu.KLTFreeTrackingContext(tc)


def child(code):
    import subprocess
    import sys
    root = str(ms.SHIM_LIB.parents[3])
    pre = ("import sys; sys.path[:0] = %r; import numpy as np, ctypes as C, kltamd\n"
           "g = kltamd.load(); g.KLTSetVerbosity(0)\n"
           "tc = g.KLTCreateTrackingContext(); fl = g.KLTCreateFeatureList(4)\n"
           "m = np.ones((64, 64), np.uint8); a = np.zeros((64, 64), np.uint8); p = a.ctypes.data_as(C.POINTER(C.c_ubyte))\n") % [root]
    return subprocess.run([sys.executable, "-c", pre + code + "\nprint('survived')\n"], capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("call", ["g.KLTSelectGoodFeatures(tc, p, 64, 48, fl)", "g.KLTTrackFeatures(tc, p, p, 64, 48, fl)"])
def test_size_mismatch_is_an_error(gpu, call):
    """A KLTError ends the process: run in a child."""
    r = child("assert g.klt_amd_set_mask(tc, m.ctypes.data, 64, 64, 3) == 0\n" + call)
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "region mask is 64 by 64, the image 64 by 48" in r.stderr


def test_tracking_use_refuses_the_forward_backward_check(gpu):
    r = child("assert g.klt_amd_set_mask(tc, m.ctypes.data, 64, 64, 2) == 0 and g.klt_amd_set_fb_check(tc, 1, 1.0) == 0\n"
              "g.KLTTrackFeatures(tc, p, p, 64, 64, fl)")
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "tracking use does not combine with the forward-backward check" in r.stderr


def test_matching_size_survives(gpu):
    r = child("assert g.klt_amd_set_mask(tc, m.ctypes.data, 64, 64, 3) == 0\n"
              "g.KLTSelectGoodFeatures(tc, p, 64, 64, fl); g.KLTTrackFeatures(tc, p, p, 64, 64, fl)\n"
              "g.KLTFreeFeatureList(fl); g.KLTFreeTrackingContext(tc)")
    assert r.returncode == 0 and "survived" in r.stdout, r.stderr[-2000:]
