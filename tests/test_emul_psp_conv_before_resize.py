"""The conv-before-resize operators (ops2d.conv_taps_split, ops2d.upsample_tapsum) on the CPU emulator:
the checks of test_gpu_psp_conv_before_resize.py at their smallest shapes, and the tap-sum kernel's reads and writes
against guard pages."""
import numpy as np
import pytest
import torch

from host_emul import emul
from psp_conv_before_resize_ref import check_layer_pair, check_tapsum

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip", "backbone2d.hip"])


@pytest.fixture
def ops2d(L, monkeypatch):
    from morefusion_amd.models import ops2d
    emul.patch_lib(L, monkeypatch)
    return ops2d


@pytest.mark.parametrize("side", [2, 4])
def test_tapsum(ops2d, side):
    check_tapsum(ops2d, "cpu", side)


@pytest.mark.parametrize("signed", [False, True])
def test_layer_pair(ops2d, signed):
    check_layer_pair(ops2d, "cpu", 1, 64, 64, signed)


def test_tapsum_stays_inside_its_buffers(L):
    """z, bias and both outputs end right in front of an inaccessible page; the odd side takes the last-row /
    last-column taps (yp = xp = 0) and a block count that is no multiple of 8"""
    B, H, W, C = 1, 3, 3, 8
    rs = np.random.RandomState(0)
    z = emul.guarded(rs.randn(B, H, W, 9 * C).astype(np.float32))
    bias = emul.guarded(rs.randn(C).astype(np.float32))
    y = emul.guarded(np.zeros((B, 2 * H, 2 * W, C), np.float32))
    ys = emul.guarded(np.zeros((B, 2 * H, 2 * W, 2 * C), np.uint16))
    assert L.mf_upsample2x_tapsum_fwd(emul.ptr(z), emul.ptr(bias), None, 1, emul.ptr(y), C, emul.ptr(ys), 2 * C, C,
                                      B, H, W, C, None) == 0
    assert np.isfinite(y).all() and (y >= 0).all() and (y > 0).any()
