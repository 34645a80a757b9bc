"""The camera-tracking entry points of the C ABI without a GPU: the sizes are host-only arithmetic and follow the
documented layout, bad arguments are refused before any launch with the library's error code, and the Python layer
refuses CPU tensors instead of falling back."""
import ctypes

import numpy as np
import pytest
import torch

import morefusion_amd as mf
from morefusion_amd.contrib import CameraTracker, align_depth

PYRAMID, ALIGN = 0, 1
INVALID = -1  # -(int)hipErrorInvalidValue


def _pyramid_bytes(B, H, W, levels):
    a16 = lambda n: (n + 15) & ~15  # noqa: E731
    off = 0
    for l in range(levels):
        n = B * (H >> l) * (W >> l)
        off = a16(a16(a16(off + 4 * n) + 24 * n) + 24 * n)
    return a16(off + 16 * levels * B)


def test_sizes_are_host_only_arithmetic_and_grow_with_every_argument():
    ws = mf._lib.lib().mf_camtrack_workspace_bytes
    for shape in ((1, 480, 640, 3), (2, 121, 163, 2), (5, 30, 40, 2), (1, 8, 8, 1)):
        assert ws(*shape, PYRAMID) == _pyramid_bytes(*shape)
    # the align workspace: 7 + 12 + 12 doubles per alignment and 32 doubles per 1024 pixels of level 0
    n = ws(1, 480, 640, 3, ALIGN)
    assert 8 * (31 + 32 * 300) <= n < 8 * (31 + 32 * 300) + 64 and n % 16 == 0
    assert ws(1, 480, 640, 1, ALIGN) == n  # the coarser levels reuse the partials of level 0
    for which in (PYRAMID, ALIGN):
        base = ws(2, 96, 128, 2, which)
        assert base > 0
        assert ws(3, 96, 128, 2, which) > base and ws(2, 128, 128, 2, which) > base
        assert ws(2, 96, 160, 2, which) > base
    assert ws(2, 96, 128, 3, PYRAMID) > ws(2, 96, 128, 2, PYRAMID)
    assert ws(2, 96, 128, 3, ALIGN) >= ws(2, 96, 128, 2, ALIGN)


def test_bad_shapes_are_refused():
    L = mf._lib.lib()
    ws = L.mf_camtrack_workspace_bytes
    assert ws(1, 32, 32, 3, PYRAMID) > 0  # 8 x 8 at the coarsest level: the smallest allowed
    for bad in ((0, 64, 64, 2, PYRAMID), (1025, 64, 64, 2, PYRAMID), (1, 64, 64, 0, PYRAMID), (1, 64, 64, 9, PYRAMID),
                (1, 31, 32, 3, PYRAMID), (1, 32, 31, 3, ALIGN), (1, 4097, 64, 2, PYRAMID), (1, 64, 64, 2, 2),
                (17, 2048, 2048, 2, ALIGN)):
        assert ws(*bad) == INVALID, bad
    assert b"mf_camtrack_workspace_bytes" in L.mf_last_error_string()


def test_prepare_and_align_validate_before_any_launch():
    L = mf._lib.lib()
    K = (100.0, 100.0, 31.5, 31.5)
    # no pointer below is ever dereferenced: the calls are refused on the host
    assert L.mf_camtrack_prepare(None, 1, 31, 32, 3, *K, 0.05, None, None) == INVALID
    assert b"mf_camtrack_prepare" in L.mf_last_error_string()
    assert L.mf_camtrack_prepare(None, 1, 64, 64, 2, 0.0, 100.0, 31.5, 31.5, 0.05, None, None) == INVALID
    assert L.mf_camtrack_prepare(None, 1, 64, 64, 2, *K, -1.0, None, None) == INVALID
    assert L.mf_camtrack_prepare(None, 1, 64, 64, 2, *K, 0.05, None, None) == INVALID  # null arrays
    iters = (ctypes.c_int32 * 2)(3, 2)
    it = ctypes.addressof(iters)
    tail = (None,) * 6
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 3, *K, None, None, it, 0.1, 0.9, 10, *tail) == INVALID  # 16 x 16, 3 levels: fine; null arrays
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 5, *K, None, None, it, 0.1, 0.9, 10, *tail) == INVALID
    assert b"mf_camtrack_align" in L.mf_last_error_string()
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, None, 0.1, 0.9, 10, *tail) == INVALID
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, it, -0.1, 0.9, 10, *tail) == INVALID
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, it, 0.1, 1.5, 10, *tail) == INVALID
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, it, 0.1, 0.9, -1, *tail) == INVALID
    negative = (ctypes.c_int32 * 2)(3, -1)
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, ctypes.addressof(negative), 0.1, 0.9, 10,
                               *tail) == INVALID
    assert b"iteration counts" in L.mf_last_error_string()
    many = (ctypes.c_int32 * 2)(4000, 4000)
    assert L.mf_camtrack_align(None, None, 1, 64, 64, 2, *K, None, None, ctypes.addressof(many), 0.1, 0.9, 10,
                               *tail) == INVALID


def test_camera_tracking_refuses_cpu_tensors_loudly():
    depth = torch.ones((32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_depth(depth, depth, np.eye(3), np.eye(4), levels=2, iterations=(1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CameraTracker(np.eye(3), 32, 32, levels=2, iterations=(1, 1), device="cpu")
