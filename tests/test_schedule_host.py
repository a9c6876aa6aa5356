"""The tail schedule's threshold arithmetic (klt_hip_tail_threshold), host only.

The pyramid stream waits until the tracker's exit count reaches the value this
function returns.  The wait can be met only by the launch it was computed for,
so the value must lie within what that launch adds: above `base` (not met
before the launch's first wave has left) and at most `base + launched` (met by
the launch's completion at the latest)."""
from __future__ import annotations

import ctypes as C

import pytest


def threshold(amd, base, launched, k):
    t = C.c_uint(0xDEADBEEF)
    wait = amd.klt_hip_tail_threshold(base, launched, k, C.byref(t))
    return wait, t.value


@pytest.mark.parametrize("base", [0, 12345, (1 << 29) + 7])
def test_threshold_lies_within_the_launch(amd, base):
    for launched in range(1, 70001):
        for k in {0, 1, 1024, launched - 1}:
            wait, t = threshold(amd, base, launched, k)
            if launched <= k:
                assert wait == 0, (launched, k)
                continue
            assert wait == 1, (launched, k)
            assert 1 <= t - base <= launched, (base, launched, k, t)
            assert t - base == launched - k


def test_no_wait_without_a_tail(amd):
    for base in (0, 99, 1 << 29):
        for k in (0, 1, 1024):
            wait, t = threshold(amd, base, 0, k)
            assert wait == 0 and t == 0xDEADBEEF  # nothing launched (n == 0): no wait, nothing written
        for launched in (1, 5, 1024):
            for k in (launched, launched + 1, 10 ** 6):
                assert threshold(amd, base, launched, k)[0] == 0


def test_null_threshold_pointer_is_allowed(amd):
    assert amd.klt_hip_tail_threshold(0, 10, 3, None) == 1
    assert amd.klt_hip_tail_threshold(0, 3, 10, None) == 0
