"""The image-only level 0 in one-wave strips (k_pyr_l0s, klt_hip_set_l0_strip).

The strip kernel and the 64x32 tiles compute the same sums in the same order,
so every plane of both levels of a kept pyramid is compared bit for bit between
the two switch positions (level 1 is built from the sigma-3.6 rows pass, hs, so
it covers that output), and a tracked sequence against the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import synth
from kltabi import OracleTracker
from test_gpu_track import assert_table_equal, batch_sequence

pytestmark = pytest.mark.gpu

F32 = np.float32

# W x H: one exact strip; a 4-pixel second strip with hsW odd (falls back to
# tiles); H shorter than a segment; 21 rows; a partial third strip and several
# segments; every lane edge or halo; ten strips of 8 rows
SHAPES = [(192, 40), (196, 37), (200, 50), (384, 21), (392, 230), (64, 12), (1920, 8)]


def kept_pyramid(gpu, frames, strips, chunk=2):
    """klt_hip_frames_begin on frames[0], a klt_hip_track_frames call over
    frames[1:] with no features, klt_hip_frames_end_slot(0): every plane of
    both levels of the last frame's pyramid."""
    from kltamd.device import H2D, PyrDesc, TrackDesc, check
    h, w = frames[0].shape
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_set_lazy_grad(ctx, 1) == 0
    assert gpu.klt_hip_set_l0_strip(ctx, strips) == 0
    stack = np.ascontiguousarray(np.stack(frames))
    dfr = gpu.klt_hip_malloc(ctx, stack.nbytes)
    check(gpu, ctx, gpu.klt_hip_memcpy(ctx, dfr, stack.ctypes.data, stack.nbytes, H2D), "h2d")
    pd, td = PyrDesc(), TrackDesc()
    gpu.klt_amd_pyr_desc(tc, w, h, tc.contents.nPyramidLevels, 1, C.byref(pd))
    gpu.klt_amd_track_desc(tc, C.byref(td))
    check(gpu, ctx, gpu.klt_hip_frames_begin(ctx, C.byref(pd), dfr, w), "begin")
    check(gpu, ctx, gpu.klt_hip_track_frames(ctx, C.byref(pd), C.byref(td), dfr + w * h, w, w * h, len(frames) - 1,
                                             chunk, None, None, None, 0, None, None, None, 0), "frames")
    check(gpu, ctx, gpu.klt_hip_frames_end_slot(ctx, 0), "end_slot")
    planes = []
    for lvl in range(tc.contents.nPyramidLevels):
        lw, lh = C.c_int(0), C.c_int(0)
        check(gpu, ctx, gpu.klt_hip_level_dims(ctx, 0, lvl, C.byref(lw), C.byref(lh)), "dims")
        for which in range(3):
            a = np.full((lh.value, lw.value), -7.0, F32)
            check(gpu, ctx, gpu.klt_hip_download_level(ctx, 0, lvl, which, a.ctypes.data), "download")
            planes.append(a)
    gpu.klt_hip_free(ctx, dfr)
    gpu.KLTFreeTrackingContext(tc)
    return planes


def assert_same_planes(got, want):
    assert len(got) == len(want) == 6
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        diff = np.argwhere(a.view(np.int32) != b.view(np.int32))
        assert len(diff) == 0, f"level {i // 3} plane {i % 3}: {len(diff)} values differ, first at (y, x) = {diff[0]}"


@pytest.mark.parametrize("nframes", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_strips_equal_tiles(gpu, w, h, nframes):
    """1, 2 and 3 frames in chunks of 2: one frame, blockIdx.z > 0, a second launch."""
    frames = synth(gpu, 1000 + w + h, w, h, nframes + 1)
    assert_same_planes(kept_pyramid(gpu, frames, 1), kept_pyramid(gpu, frames, 0))


def test_width_no_multiple_of_4(gpu):
    """333x251 keeps the tiles whatever the switch says."""
    frames = synth(gpu, 335, 333, 251, 4)
    assert_same_planes(kept_pyramid(gpu, frames, 1), kept_pyramid(gpu, frames, 0))


def test_setter(gpu):
    """The setter takes 0 and 1 and refuses a null context."""
    tc = gpu.KLTCreateTrackingContext()
    ctx = gpu.klt_amd_device_context(tc)
    assert gpu.klt_hip_set_l0_strip(ctx, 0) == 0
    assert gpu.klt_hip_set_l0_strip(ctx, 1) == 0
    assert gpu.klt_hip_set_l0_strip(None, 1) != 0
    gpu.KLTFreeTrackingContext(tc)


@pytest.fixture(scope="module")
def seq640(gpu, oracle):
    frames = synth(gpu, 5150, 640, 480, 12)
    return frames, OracleTracker(oracle).harness(frames, 300, 12, first=frames[0])


@pytest.mark.parametrize("chunk", [5, 12])
def test_tracked_run(gpu, seq640, chunk):
    """640x480, 300 features, 12 frames: the table rows with strips equal the
    rows with tiles and the oracle's."""
    frames, want = seq640
    tables = []
    for strips in (1, 0):
        def hook(ctx, done=False, strips=strips):
            if not done:
                assert gpu.klt_hip_set_l0_strip(ctx, strips) == 0
        tables.append(batch_sequence(gpu, frames, 300, [chunk], ctx_hook=hook))
    for a, b in zip(tables[0], tables[1]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert_table_equal(*tables[0], *want)
