"""Pixel formats of device frames, the host side (klt_hip_frame_bpp,
klt_hip_gray_host): no device needed.

The definition (include/klt_hip.h): gray = (4899 R + 9617 G + 1868 B + 8192) >> 14
in integers, alpha ignored.  The expected values here are that formula in numpy
uint32, never the library's own output.
"""
from __future__ import annotations

import numpy as np
import pytest

from kltamd.device import FRAME_BGR8, FRAME_BGRA8, FRAME_GRAY8, FRAME_RGB8, FRAME_RGBA8

COLOUR = [FRAME_RGB8, FRAME_BGR8, FRAME_RGBA8, FRAME_BGRA8]
BPP = {FRAME_GRAY8: 1, FRAME_RGB8: 3, FRAME_BGR8: 3, FRAME_RGBA8: 4, FRAME_BGRA8: 4}


def gray_np(r, g, b):
    r, g, b = (np.asarray(c).astype(np.uint32) for c in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def pack(fmt, r, g, b, alpha=None, pad=0, fill=0xA5):
    """[H, W] channels as one [H, W * bpp + pad] byte image of `fmt`."""
    h, w = r.shape
    bpp = BPP[fmt]
    px = np.empty((h, w, bpp), np.uint8)
    first, last = (b, r) if fmt in (FRAME_BGR8, FRAME_BGRA8) else (r, b)
    px[..., 0], px[..., 1], px[..., 2] = first, g, last
    if bpp == 4:
        px[..., 3] = 255 if alpha is None else alpha
    out = np.full((h, w * bpp + pad), fill, np.uint8)
    out[:, :w * bpp] = px.reshape(h, w * bpp)
    return out


def gray_host(amd, fmt, src, w, h, pitch=None, dst_pitch=None):
    dst_pitch = w if dst_pitch is None else dst_pitch
    dst = np.full((h, dst_pitch), 0x5A, np.uint8)
    rc = amd.klt_hip_gray_host(fmt, src.ctypes.data, src.shape[1] if pitch is None else pitch, w, h, dst.ctypes.data,
                               dst_pitch)
    return rc, dst


def sweeps():
    """256x3 per channel: the channel runs 0..255 with the others at 0, then at 255."""
    ramp = np.tile(np.arange(256, dtype=np.uint8), (1, 1))
    cases = []
    for other in (0, 255):
        rows = []
        for ch in range(3):
            rgb = [np.full((1, 256), other, np.uint8) for _ in range(3)]
            rgb[ch] = ramp
            rows.append(rgb)
        cases.append(tuple(np.concatenate([row[k] for row in rows]) for k in range(3)))
    return cases


def test_bytes_per_pixel(amd):
    assert [amd.klt_hip_frame_bpp(f) for f in range(5)] == [1, 3, 3, 4, 4]
    for bad in (-1, 5, 1000):
        assert amd.klt_hip_frame_bpp(bad) == -1


def test_weights_sum_to_one():
    assert gray_np(255, 255, 255) == 255 and gray_np(0, 0, 0) == 0
    v = np.arange(256)
    assert np.array_equal(gray_np(v, v, v), v)


@pytest.mark.parametrize("fmt", COLOUR)
def test_random_triples(amd, fmt):
    rng = np.random.default_rng(7)
    r, g, b = (rng.integers(0, 256, (4, 64), dtype=np.uint8) for _ in range(3))
    rc, got = gray_host(amd, fmt, pack(fmt, r, g, b), 64, 4)
    assert rc == 0
    assert np.array_equal(got, gray_np(r, g, b))


@pytest.mark.parametrize("fmt", COLOUR)
def test_channel_sweeps(amd, fmt):
    for r, g, b in sweeps():
        rc, got = gray_host(amd, fmt, pack(fmt, r, g, b), 256, 3)
        assert rc == 0
        assert np.array_equal(got, gray_np(r, g, b))


@pytest.mark.parametrize("fmt", COLOUR)
def test_padded_pitches(amd, fmt):
    rng = np.random.default_rng(8)
    r, g, b = (rng.integers(0, 256, (4, 64), dtype=np.uint8) for _ in range(3))
    rc, got = gray_host(amd, fmt, pack(fmt, r, g, b, pad=7), 64, 4, dst_pitch=64 + 5)
    assert rc == 0
    assert np.array_equal(got[:, :64], gray_np(r, g, b))
    assert (got[:, 64:] == 0x5A).all()  # the padding of dst is not written


@pytest.mark.parametrize("fmt", [FRAME_RGBA8, FRAME_BGRA8])
def test_alpha_is_ignored(amd, fmt):
    rng = np.random.default_rng(9)
    r, g, b, a = (rng.integers(0, 256, (4, 64), dtype=np.uint8) for _ in range(4))
    want = gray_np(r, g, b)
    for alpha in (0, 255, a):
        rc, got = gray_host(amd, fmt, pack(fmt, r, g, b, alpha=alpha), 64, 4)
        assert rc == 0 and np.array_equal(got, want)


def test_channel_order_matters(amd):
    rng = np.random.default_rng(10)
    r, g, b = (rng.integers(0, 256, (4, 64), dtype=np.uint8) for _ in range(3))
    src = pack(FRAME_RGB8, r, g, b)
    _, as_rgb = gray_host(amd, FRAME_RGB8, src, 64, 4)
    _, as_bgr = gray_host(amd, FRAME_BGR8, src, 64, 4)
    assert np.array_equal(as_bgr, gray_np(b, g, r)) and not np.array_equal(as_rgb, as_bgr)


def test_gray_copies(amd):
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (5, 37 + 3), dtype=np.uint8)
    rc, got = gray_host(amd, FRAME_GRAY8, f, 37, 5, dst_pitch=41)
    assert rc == 0
    assert np.array_equal(got[:, :37], f[:, :37]) and (got[:, 37:] == 0x5A).all()


def test_refusals(amd):
    src = np.zeros((4, 64 * 4), np.uint8)
    for bad in (-1, 5):
        rc, got = gray_host(amd, bad, src, 64, 4)
        assert rc == -1 and (got == 0x5A).all()
    for fmt in [FRAME_GRAY8] + COLOUR:
        rc, got = gray_host(amd, fmt, src, 64, 4, pitch=64 * BPP[fmt] - 1)
        assert rc == -1 and (got == 0x5A).all()
        rc, got = gray_host(amd, fmt, src, 64, 4, pitch=64 * BPP[fmt])
        assert rc == 0
    dst = np.zeros((4, 64), np.uint8)
    assert amd.klt_hip_gray_host(FRAME_RGB8, src.ctypes.data, 192, 64, 4, dst.ctypes.data, 63) == -1
    assert amd.klt_hip_gray_host(FRAME_RGB8, None, 192, 64, 4, dst.ctypes.data, 64) == -1
    assert amd.klt_hip_gray_host(FRAME_RGB8, src.ctypes.data, 192, 64, 4, None, 64) == -1
