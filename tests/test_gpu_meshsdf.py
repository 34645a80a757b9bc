"""Mesh signed distance / solid voxelization on the MI355X (csrc/meshsdf.hip through geometry.mesh_sdf and
datasets.YCBVideoModels): the three real YCB meshes bit for bit against the NumPy mirror (tests/meshsdf_ref.py)
-- solid-grid occupancy, the get_sdf point sets and random points in the padded bbox --, a batched launch against
one launch per mesh, degenerate faces and empty query sets, get_sdf against the reference's own fixture clouds,
and ICC on fixture 0 with the mesh-derived (points, sdf)."""
import os

import numpy as np
import pytest
import torch

import meshsdf_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.geometry import mesh_sdf  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("003_cracker_box", "004_sugar_box", "010_potted_meat_can")
CLASS_OF = {2: "003_cracker_box", 3: "004_sugar_box", 9: "010_potted_meat_can"}
WORKERS = 8


def _mesh(name):
    d = np.load(os.path.join(GOLDEN, f"ycb_mesh_{name}.npz"))
    return d["vertices"], d["faces"]


def _np(x):
    return x.cpu().numpy()


def _same(got, ref, check_w=True):
    assert np.array_equal(_np(got["dist"]), ref["dist"])
    assert np.array_equal(_np(got["face"]), ref["face"])
    assert np.array_equal(_np(got["sdf"]), ref["sdf"])
    np.testing.assert_allclose(_np(got["winding"]), ref["winding"], rtol=0, atol=1e-12)
    if check_w:
        decided = ref["dist"] > R.ON_SURFACE
        assert not (np.abs(ref["winding"][decided] - 0.5) < 1e-9).any()


@pytest.fixture(scope="module")
def grids():
    meshes = [_mesh(n) for n in NAMES]
    return meshes, mesh_sdf.solid_voxel_grid_batch(meshes, 64)


def _tree(root):
    """A YCBVideoModels tree of the three committed meshes (OBJ text of their exact float64 values)."""
    for name in NAMES:
        v, f = _mesh(name)
        (root / name).mkdir()
        text = "".join(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in v)
        text += "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)
        (root / name / "textured.obj").write_text(text)
    return morefusion.datasets.YCBVideoModels(root)


@pytest.mark.parametrize("m", range(3))
def test_solid_grid_occupancy_bitwise_vs_mirror(grids, m):
    meshes, g = grids
    v, f = meshes[m]
    origin, h = R.grid_params(v, 64)
    assert np.array_equal(_np(g[m].origin), origin) and g[m].pitch == h
    occ = _np(g[m].matrix).reshape(-1)
    assert 0.05 < occ.mean() < 0.9
    # the mirror on every cell that differs from a face neighbour (the surface layer) and on 3000 random cells
    o = occ.reshape(64, 64, 64)
    edge = np.zeros_like(o)
    for a in range(3):
        d = np.diff(o.astype(np.int8), axis=a) != 0
        sl_lo = [slice(None)] * 3
        sl_hi = [slice(None)] * 3
        sl_lo[a], sl_hi[a] = slice(0, 63), slice(1, 64)
        edge[tuple(sl_lo)] |= d
        edge[tuple(sl_hi)] |= d
    rs = np.random.RandomState(m)
    idx = np.flatnonzero(edge.reshape(-1))
    idx = np.union1d(rs.choice(idx, min(len(idx), 5000), replace=False), rs.choice(64 ** 3, 3000, replace=False))
    ref, _, _, _ = R.solid_occupancy(v, f, 64, index=idx, workers=WORKERS)
    assert np.array_equal(occ[idx], ref)
    assert np.array_equal(_np(g[m].points), R.grid_centres(origin, h, 64, np.flatnonzero(occ)))


def test_queries_bitwise_vs_mirror_and_batch_equals_single(grids):
    meshes, g = grids
    rs = np.random.RandomState(5)
    pts = []
    for (v, f), gr in zip(meshes, g):
        lo, hi = v.min(0), v.max(0)
        solid = morefusion.extra.open3d.voxel_down_sample(gr.points, gr.pitch * 2)
        pts.append(torch.cat([solid, torch.from_numpy(rs.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo),
                                                                  (1500, 3))).cuda()]))
    batch = mesh_sdf.mesh_signed_distance_batch(meshes, pts)
    for (v, f), p, got in zip(meshes, pts, batch):
        ref = R.signed_distance(v, f, _np(p), workers=WORKERS)
        _same(got, ref)
        one = mesh_sdf.mesh_signed_distance_batch([(v, f)], [p])[0]
        for k in got:
            assert torch.equal(one[k], got[k])
        assert (ref["sdf"][:len(p) - 1500] > 0).mean() > 0.8  # most solid points lie inside (surface cells need not)
    # NumPy in, NumPy out; tensors in, device tensors out
    v, f = meshes[0]
    sdf_np = mesh_sdf.mesh_signed_distance(v, f, _np(pts[0]))
    sdf_t = mesh_sdf.mesh_signed_distance(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), pts[0])
    assert isinstance(sdf_np, np.ndarray) and sdf_t.is_cuda and np.array_equal(sdf_np, _np(sdf_t))
    assert np.array_equal(sdf_np, _np(batch[0]["sdf"]))


def test_degenerate_faces_and_empty_query_sets():
    bv, bf = R.box_mesh()
    bv = np.vstack([bv, [[0.5, 0.5, 2.0], [0.5, 0.5, 3.0], [0.5, 0.5, 4.0]]])
    bf = np.vstack([bf, [[8, 8, 9], [8, 9, 10], [10, 10, 10], [0, 0, 7]]]).astype(np.int32)
    ico = R.icosphere(2, 0.4)
    p = np.random.RandomState(1).uniform(-0.5, 4.5, (700, 3))
    out = mesh_sdf.mesh_signed_distance_batch([(bv, bf), ico, (bv, bf)],
                                              [torch.zeros((0, 3)).cuda(), torch.from_numpy(p[:5]).cuda(),
                                               torch.from_numpy(p).cuda()])
    assert out[0]["sdf"].shape == (0,)
    _same(out[1], R.signed_distance(*ico, p[:5]))
    _same(out[2], R.signed_distance(bv, bf, p))


def test_get_sdf_vs_reference_fixture_clouds(tmp_path):
    from scipy.spatial import cKDTree
    ycb = _tree(tmp_path)
    ids = [ycb.class_names.index(CLASS_OF[int(np.load(os.path.join(GOLDEN, f"fixture_pose_refinement_0000000{i}.npz"))
                                                   ["class_id"])]) for i in range(3)]
    res = ycb.get_sdf_batch(ids)
    for i, (pts, sdf) in enumerate(res):
        fx = np.load(os.path.join(GOLDEN, f"fixture_pose_refinement_0000000{i}.npz"))
        ref = fx["pcd_cad"].astype(np.float64)
        pitch = ycb.get_voxel_pitch(32, ids[i])
        assert pts.dtype == np.float64 and sdf.dtype == np.float64 and pts.shape == (len(sdf), 3)
        assert abs(len(pts) / len(ref) - 1) <= 0.05, (len(pts), len(ref))
        d = 0.5 * (cKDTree(ref).query(pts)[0].mean() + cKDTree(pts).query(ref)[0].mean())
        assert d <= 0.15 * pitch, (d / pitch)
        assert (sdf > 0).mean() > 0.9 and sdf.max() < 0.5 * ycb.get_bbox_diagonal(ids[i])
        print(f"fixture {i}: {len(pts)} points (reference {len(ref)}), mean NN distance {d / pitch:.3f} pitch")
    # the cache file has the reference's keys and loads in a fresh instance
    data = np.load(tmp_path / NAMES[ids[0] - 1] / "sdf.npz")
    assert set(data.files) == {"points", "sdf"} and np.array_equal(data["sdf"], res[0][1])
    again = morefusion.datasets.YCBVideoModels(tmp_path).get_sdf(ids[0])
    assert np.array_equal(again[0], res[0][0])
    # one class alone == its row of the batch
    (tmp_path / "b").mkdir()
    fresh = _tree(tmp_path / "b")
    solo = fresh.get_sdf(ids[2])
    assert np.array_equal(solo[0], res[2][0]) and np.array_equal(solo[1], res[2][1])


def test_icc_fixture0_with_mesh_sdf(tmp_path):
    """The reference node's ICC (Adam 0.01, translation x0.1, 30 steps) on fixture 0 with get_sdf's CAD data."""
    fx = np.load(os.path.join(GOLDEN, "fixture_pose_refinement_00000000.npz"))
    ycb = _tree(tmp_path)
    pts, sdf = ycb.get_sdf(ycb.class_names.index(CLASS_OF[int(fx["class_id"])]))
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    args = ([d(pts.astype(np.float32))], [d(sdf.astype(np.float32))], d(np.asarray([fx["pitch"]], np.float32)),
            d(fx["origin"][None].astype(np.float32)), d(fx["grid_target"][None].astype(np.float32)),
            d(fx["grid_nontarget_empty"][None].astype(np.float32)))
    link = morefusion.contrib.IterativeCollisionCheckLink(fx["transform_init"][None].astype(np.float32),
                                                          sdf_offset=0.02).to_gpu()
    opt = morefusion.optimizers.Adam(alpha=0.01).setup(link)
    link.translation.update_rule.hyperparam.alpha *= 0.1
    losses = []
    for _ in range(30):
        loss = link(*args)
        loss.backward()
        opt.update()
        link.zerograds()
        losses.append(float(loss.detach()))
    print("ICC losses", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] <= losses[0]
