"""The front end's kernel (mf_maxpool3s2_split_fwd) and res2 / res3's layer forms on the CPU emulator:
the checks of test_gpu_frontend_split.py, and the new kernel's reads and writes against guard pages."""
import numpy as np
import pytest
import torch

from host_emul import emul
import frontend_split_ref as R

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def L():
    return emul.build(["gemm_bf16.hip", "backbone2d.hip"])


@pytest.fixture
def ops2d(L, monkeypatch):
    from morefusion_amd.models import ops2d
    emul.patch_lib(L, monkeypatch)
    return ops2d


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("side", [8, 16])
@pytest.mark.parametrize("kind", ["negative", "border"])
def test_maxpool(ops2d, kind, side, channels_last):
    R.check_maxpool(ops2d, "cpu", kind, side, channels_last)


@pytest.mark.parametrize("name", list(R.FRONT_LAYERS))
def test_front_layer(ops2d, name):
    R.check_front_layer(ops2d, "cpu", name, 1)


def test_maxpool_stays_inside_its_buffers(L):
    """an odd side (the last window hangs over the right / bottom border), a strip that is not full and a channel
    count below the workgroup's 64: x and both outputs end right in front of an inaccessible page"""
    B, C, H, W = 1, 8, 7, 7
    rs = np.random.RandomState(0)
    x = emul.guarded(rs.randn(B, C, H, W).astype(np.float32))
    y = emul.guarded(np.zeros((B, 4, 4, C), np.float32))
    ys = emul.guarded(np.zeros((B, 4, 4, 2 * C), np.uint16))
    assert L.mf_maxpool3s2_split_fwd(emul.ptr(x), C * H * W, H * W, W, 1, B, C, H, W, emul.ptr(y), emul.ptr(ys), None) == 0
    want = torch.nn.functional.max_pool2d(torch.from_numpy(np.array(x)), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(y, want)
    assert L.mf_maxpool3s2_split_fwd(emul.ptr(x), C * H * W, H * W, W, 1, B, 12, H, W, emul.ptr(y), None, None) != 0
