"""conv3's occupancy channels on the split-bf16 path on the CPU emulator: the checks of
test_gpu_volumetric_split2.py on the emulated kernels, the second occupancy convolution's split store against guard
pages, and the launch plan of the layer's real shape (host arithmetic)."""
import ctypes

import numpy as np
import pytest

from host_emul import emul
import volumetric_split2_ref as R

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def L():
    return emul.build(["conv3d.hip", "gemm_bf16.hip", "backbone2d.hip"])


@pytest.fixture(params=list(R.FORMS))
def form(request, monkeypatch):
    for k in ("MF_NT_BIG", "MF_NT_SPLITK", "MF_NT_HALF_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in R.FORMS[request.param][0].items():
        monkeypatch.setenv(k, v)
    return request.param


def test_occupancy_split_store(L):
    R.check_occupancy_split_store(L, "cpu", None)


def test_occupancy_split_store_stays_inside_its_buffers(L):
    """343 voxels = one full and one ragged workgroup; the grid, the scratch and the split output (alone: no fp32
    store) end right in front of an inaccessible page"""
    B, Dg = 1, 7
    grid, w1, b1, w2, b2 = (t.numpy() for t in R.occupancy_problem(B, Dg, seed=5))
    n = B * Dg ** 3
    g = emul.guarded(grid)
    h1 = emul.guarded(np.zeros((n, 8), np.float32))
    h2 = np.zeros((n, 16), np.float32)
    assert L.mf_occupancy_convs_fwd(emul.ptr(g), emul.ptr(w1), emul.ptr(b1), emul.ptr(w2), emul.ptr(b2), emul.ptr(h1),
                                    emul.ptr(h2), B, Dg, None) == 0
    h2s = emul.guarded(np.zeros((n, 32), np.uint16))
    assert L.mf_occupancy_convs_split_fwd(emul.ptr(g), emul.ptr(w1), emul.ptr(b1), emul.ptr(w2), emul.ptr(b2),
                                          emul.ptr(h1), None, emul.ptr(h2s), B, Dg, None) == 0
    import torch
    want = R.bits(R.split(torch.from_numpy(h2))).numpy().view(np.uint16)
    assert np.array_equal(np.array(h2s), want) and (want[:, 16:] != 0).mean() > 0.2


@pytest.mark.parametrize("B", [1, 2])
def test_conv3_occ_error_bound(L, form, B):
    R.check_conv3_occ_bound(L, "cpu", None, form, B)


def test_conv3_occ_single_voxel_single_tap(L, form):
    R.check_single_voxel_single_tap(L, "cpu", None, form)


@pytest.mark.parametrize("B,tile,S", [(8, 256, 2), (4, 256, 3)])
def test_conv3_occ_plan_at_the_real_shape(L, monkeypatch, B, tile, S):
    """32^3 -> 16^3, Cin 16, Cout 256: M = B 4096 rows, K = 64 taps x 48.  8 objects: 128 tiles of 256 x 256, the 48
    K-tiles in two halves; the workspace query answers for the same plan."""
    for k in ("MF_NT_BIG", "MF_NT_SPLITK", "MF_NT_HALF_MAX"):
        monkeypatch.delenv(k, raising=False)
    t, s = ctypes.c_int32(0), ctypes.c_int32(0)
    M = B * 16 ** 3
    assert L.mf_gemm_bf16_nt_plan(R.MODE_CONV3_SPLIT, M, R.COUT, 64 * 3 * R.CIN, 1, 0, 0, 1, 1, ctypes.byref(t),
                                  ctypes.byref(s)) == 0
    assert (t.value, s.value) == (tile, S)
    assert L.mf_conv3d_k4s2_split_workspace_bytes(B, R.CIN, R.COUT, 32) == S * M * R.COUT * 4
