"""The TSDF mesh on the MI355X (csrc/tsdfmesh.hip through contrib.TsdfVolume.extract_mesh) against the NumPy mirror
(tests/tsdfmesh_ref.py), bit for bit: the cases (a) .. (f) of tests/tsdfmesh_cases.py; one 480 x 640 frame fused into
the 64^3 volume of tests/test_gpu_tsdf.py; run-to-run identity; and the mesh rendered by geometry.render_meshes
against TsdfVolume.raycast from the same pose."""
import numpy as np
import pytest
import torch

import camtrack_cases as CC
import tsdfmesh_cases as C
from morefusion_amd import _lib, geometry
from morefusion_amd.contrib import TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,min_weight", [("a", 1.0), ("a", 2.0), ("b", 1.0), ("c", 1.0), ("d", 1.0), ("e", 1.0)])
def test_cases_bitwise_vs_mirror(name, min_weight):
    case = C.make_case(name)
    exp = C.run_mirror(case, min_weight)
    assert len(exp["faces"]) > 0
    C.assert_equal(C.run_product(case, "cuda", min_weight), exp)


@pytest.mark.parametrize("name", ["f_fresh", "f_positive"])
def test_f_no_surface_gives_empty_tensors_and_no_emit_launch(monkeypatch, name):
    lib = C.CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    got = C.run_product(C.make_case(name), "cuda")
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["normals"].shape == (0, 3)
    assert lib.calls["mf_tsdfmesh_count"] == 2 and "mf_tsdfmesh_emit" not in lib.calls


@pytest.fixture(scope="module")
def full_frames():
    return CC.sequence(0, 2, 480, 640)


@pytest.fixture(scope="module")
def full_volume(full_frames):
    f0 = full_frames[0]
    vol = TsdfVolume(**C.FULL_VOLUME)
    vol.integrate(torch.as_tensor(f0["depth"]).cuda(), f0["K"], f0["T_sensor_to_map"])
    return vol


def _bytes(vol):
    return [t.cpu().numpy().tobytes() for t in vol.extract_mesh(normals=True)]


def test_full_frame_in_64_cubed_bitwise_vs_mirror_and_run_to_run(full_frames, full_volume):
    case, ref = C.full_volume_mirror(full_frames)
    assert np.array_equal(full_volume.volume.cpu().numpy(), ref.volume)
    exp = C.run_mirror(case)
    v, f, n = full_volume.extract_mesh(normals=True)
    C.assert_equal(dict(vertices=v.cpu().numpy(), faces=f.cpu().numpy(), normals=n.cpu().numpy()), exp)
    assert len(exp["faces"]) > 10000
    # two identical call sequences, the second on a volume built again from the frame
    again = TsdfVolume(**C.FULL_VOLUME)
    again.integrate(torch.as_tensor(full_frames[0]["depth"]).cuda(), full_frames[0]["K"],
                    full_frames[0]["T_sensor_to_map"])
    assert _bytes(full_volume) == _bytes(again)


def test_the_rendered_mesh_is_the_raycast_of_the_volume(full_frames, full_volume):
    """Frame 1's pose: where the render of the mesh and the ray-cast of the volume both have a depth, the median
    absolute difference is below one pitch (the bound tests/test_gpu_tsdf.py uses for ray-cast against frame; the
    two mirrors give a median of 0 -- on the scene's planes the tsdf is linear and 76 % of the 139 459 pixels agree to
    the float32 bit -- with the 90th percentile at 0.064 pitch and the 99th at 0.69 pitch, DESIGN.md "TSDF mesh")."""
    f0, f1 = full_frames
    T1 = np.asarray(f1["T_sensor_to_map"], np.float64)
    vertices, faces = full_volume.extract_mesh()
    out = geometry.render_meshes([(vertices, faces)], [np.linalg.inv(T1)], f0["K"], 480, 640)
    rendered = out["depth"][0].cpu().numpy()
    ray = full_volume.raycast(f0["K"], torch.as_tensor(T1).cuda(), 480, 640).cpu().numpy()
    both = ~np.isnan(rendered) & (ray > 0)
    assert both.mean() > 0.25
    median = float(np.median(np.abs(rendered[both] - ray[both])))
    print("median |render - raycast| =", median, "m =", median / C.FULL_VOLUME["pitch"], "pitch")
    assert median < C.FULL_VOLUME["pitch"]
