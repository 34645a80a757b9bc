"""csrc/tsdfmesh.hip through the host emulator behind the product's Python layer (contrib.TsdfVolume.extract_mesh;
torch CPU tensors as device memory): vertices, faces and normals of the cases (a) .. (f) of tests/tsdfmesh_cases.py
bitwise equal to the NumPy mirror (tests/tsdfmesh_ref.py; tests/test_tsdfmesh_host.py asserts what the mirror's meshes
are), every buffer fenced by an inaccessible page, and the Python layer's own refusals."""
import ctypes

import numpy as np
import pytest
import torch

import tsdfmesh_cases as C
from host_emul import emul
from morefusion_amd import _lib
from morefusion_amd.contrib import TsdfVolume

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def product(monkeypatch):
    lib = C.CountingLib(emul.build(["tsdfmesh.hip"]))
    emul.patch_lib(lib, monkeypatch)
    return lib


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_cases_bitwise_vs_mirror(product, name):
    case = C.make_case(name)
    exp = C.run_mirror(case)
    assert len(exp["faces"]) > 0
    C.assert_equal(C.run_product(case, "cpu"), exp)
    assert product.calls["mf_tsdfmesh_count"] == 2 and product.calls["mf_tsdfmesh_emit"] == 2


def test_a_with_min_weight_2_has_strictly_fewer_faces(product):
    case = C.make_case("a")
    got = C.run_product(case, "cpu", min_weight=2.0)
    C.assert_equal(got, C.run_mirror(case, min_weight=2.0))
    assert 0 < len(got["faces"]) < len(C.run_mirror(case)["faces"])


@pytest.mark.parametrize("name", ["f_fresh", "f_positive"])
def test_f_no_surface_gives_empty_tensors_and_no_emit_launch(product, name):
    got = C.run_product(C.make_case(name), "cpu")
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["normals"].shape == (0, 3)
    assert product.calls["mf_tsdfmesh_count"] == 2 and "mf_tsdfmesh_emit" not in product.calls


@pytest.mark.parametrize("side", ["after", "before"])
def test_no_kernel_touches_a_byte_outside_its_buffers(monkeypatch, side):
    """Cases d (chunks of a row, the column behind a chunk) and a (odd sizes: the flags kernel's tail) with every
    tensor in a mapping fenced by an inaccessible page."""
    L = emul.build(["tsdfmesh.hip"])
    for name in ("d", "a"):
        case = C.make_case(name)
        with emul.GuardedTensors(L, side=side) as guarded:
            emul.patch_lib(guarded, monkeypatch)
            got = C.run_product(case, "cpu")
        C.assert_equal(got, C.run_mirror(case))


def test_extract_mesh_refuses_a_min_weight_that_is_not_positive(product):
    vol = C.volume_of(C.make_case("e"), "cpu")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="min_weight"):
            vol.extract_mesh(min_weight=bad)
    assert not product.calls


def test_extract_mesh_refuses_totals_of_2_to_the_31(monkeypatch):
    """A library whose count reports 2^31 vertices (no real volume can be that large in a test): ValueError, and no
    emit."""
    real = emul.build(["tsdfmesh.hip"])
    calls = []

    class Huge:
        mf_tsdfmesh_workspace_bytes = staticmethod(real.mf_tsdfmesh_workspace_bytes)

        @staticmethod
        def mf_tsdfmesh_count(volume, nx, ny, nz, min_weight, workspace, totals, stream):
            (ctypes.c_int64 * 2).from_address(totals)[:] = [1 << 31, 7]
            return 0

        @staticmethod
        def mf_tsdfmesh_emit(*args):
            calls.append(args)
            return 0

    emul.patch_lib(Huge, monkeypatch)
    vol = TsdfVolume((3, 3, 3), 0.1, (0, 0, 0), device="cpu")
    with pytest.raises(ValueError, match="2\\^31"):
        vol.extract_mesh()
    assert not calls


def test_workspace_is_two_bytes_a_point_and_sixteen_a_row():
    L = emul.build(["tsdfmesh.hip"])
    assert L.mf_tsdfmesh_workspace_bytes(23, 19, 17) == 2 * ((23 * 19 * 17 + 15) // 16 * 16) + (19 * 17 + 1) * 16
    assert L.mf_tsdfmesh_workspace_bytes(256, 256, 256) == 2 * 256 ** 3 + (256 * 256 + 1) * 16
    assert L.mf_tsdfmesh_workspace_bytes(1, 8, 8) < 0 and L.mf_tsdfmesh_workspace_bytes(2048, 1024, 1024) < 0


def test_emit_leaves_rows_past_the_given_totals_alone():
    """mf_tsdfmesh_emit with smaller totals than the count's writes the leading rows only."""
    L = emul.build(["tsdfmesh.hip"])
    case = C.make_case("b")
    exp = C.run_mirror(case)
    vol = torch.from_numpy(case["volume"]).contiguous()
    nz, ny, nx = vol.shape[:3]
    ws = torch.zeros(L.mf_tsdfmesh_workspace_bytes(nx, ny, nz) // 8 + 2, dtype=torch.float64)
    totals = torch.zeros(2, dtype=torch.int64)
    assert L.mf_tsdfmesh_count(vol.data_ptr(), nx, ny, nz, 1.0, ws.data_ptr(), totals.data_ptr(), None) == 0
    V, F = totals.tolist()
    assert (V, F) == (len(exp["vertices"]), len(exp["faces"]))
    v = torch.full((V, 3), -7.0, dtype=torch.float64)
    f = torch.full((F, 3), -7, dtype=torch.int32)
    o = [float(x) for x in case["origin"]]
    assert L.mf_tsdfmesh_emit(vol.data_ptr(), nx, ny, nz, *o, case["pitch"], 1.0, ws.data_ptr(), V - 10, F - 10,
                              v.data_ptr(), f.data_ptr(), None, None) == 0
    assert np.array_equal(v.numpy()[:V - 10], exp["vertices"][:V - 10]) and (v.numpy()[V - 10:] == -7).all()
    assert np.array_equal(f.numpy()[:F - 10], exp["faces"][:F - 10]) and (f.numpy()[F - 10:] == -7).all()
