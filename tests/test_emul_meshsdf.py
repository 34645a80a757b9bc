"""csrc/meshsdf.hip through the host emulator (tests/host_emul) behind the product's Python layer
(geometry/mesh_sdf.py, torch CPU tensors as device memory): a box, an icosphere and a query sub-sample of one
YCB mesh, batched, bitwise equal to the NumPy mirror (tests/meshsdf_ref.py) -- distance, face, sdf and
occupancy; the winding number to 1e-12."""
import os

import numpy as np
import pytest
import torch

import meshsdf_ref as R
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def M(monkeypatch):
    from morefusion_amd.geometry import mesh_sdf as mod
    L = emul.build(["meshsdf.hip"])
    emul.patch_lib(L, monkeypatch)
    return mod


def _ycb(name):
    d = np.load(os.path.join(GOLDEN, f"ycb_mesh_{name}.npz"))
    return d["vertices"], d["faces"]


def _same(got, ref):
    assert np.array_equal(got["dist"].numpy(), ref["dist"])
    assert np.array_equal(got["face"].numpy(), ref["face"])
    assert np.array_equal(got["sdf"].numpy(), ref["sdf"])
    np.testing.assert_allclose(got["winding"].numpy(), ref["winding"], rtol=0, atol=1e-12)
    decided = ref["dist"] > R.ON_SURFACE  # the sign rests on w there
    assert not (np.abs(ref["winding"][decided] - 0.5) < 1e-9).any()


def test_batch_box_icosphere_ycb_bitwise_vs_mirror(M):
    rs = np.random.RandomState(0)
    box = R.box_mesh((-0.1, 0.0, 0.2), (0.3, 0.25, 0.45))
    ico = R.icosphere(2, 0.2)
    ycb = _ycb("004_sugar_box")
    lo, hi = ycb[0].min(0), ycb[0].max(0)
    pts = [rs.uniform(-0.3, 0.6, (300, 3)), rs.uniform(-0.3, 0.3, (257, 3)),
           rs.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (96, 3))]
    meshes = [box, ico, ycb]
    got = M.mesh_signed_distance_batch(meshes, [torch.from_numpy(p) for p in pts], device="cpu")
    for (v, f), p, g in zip(meshes, pts, got):
        _same(g, R.signed_distance(v, f, p))
    # the single-mesh form: NumPy in, NumPy out
    sdf, d, fid, w = M.mesh_signed_distance(*box, pts[0], return_distance=True, return_face=True,
                                            return_winding=True, device="cpu")
    assert isinstance(sdf, np.ndarray) and np.array_equal(sdf, got[0]["sdf"].numpy()) and fid.dtype == np.int32
    np.testing.assert_allclose(sdf, R.box_sdf(pts[0], (-0.1, 0.0, 0.2), (0.3, 0.25, 0.45)), rtol=0, atol=1e-12)


def test_solid_grid_and_degenerate_faces(M):
    v, f = R.icosphere(1, 0.5)
    g = M.solid_voxel_grid(v, f, dimension=12, device="cpu")
    occ, origin, h, _ = R.solid_occupancy(v, f, 12)
    assert np.array_equal(g.matrix.reshape(-1), occ) and g.pitch == h and np.array_equal(g.origin, origin)
    assert np.array_equal(g.points, R.grid_centres(origin, h, 12, np.flatnonzero(occ)))
    # zero-area faces (a repeated vertex, three collinear vertices, one point) and an empty query set
    bv, bf = R.box_mesh()
    bv = np.vstack([bv, [[0.5, 0.5, 2.0], [0.5, 0.5, 3.0], [0.5, 0.5, 4.0]]])
    bf = np.vstack([bf, [[8, 8, 9], [8, 9, 10], [10, 10, 10], [0, 0, 7]]]).astype(np.int32)
    p = np.random.RandomState(1).uniform(-0.5, 4.5, (200, 3))
    got, empty = M.mesh_signed_distance_batch([(bv, bf), (bv, bf)], [torch.from_numpy(p), torch.zeros((0, 3))],
                                              device="cpu")
    ref = R.signed_distance(bv, bf, p)
    _same(got, ref)
    assert empty["sdf"].shape == (0,)
    segment = np.linalg.norm(p - np.stack([np.full(200, 0.5), np.full(200, 0.5), np.clip(p[:, 2], 2, 4)], 1), axis=1)
    np.testing.assert_array_equal(ref["dist"], np.minimum(np.abs(R.box_sdf(p, (0, 0, 0), (1, 1, 1))), segment))
