"""The mesh-SDF mirror (tests/meshsdf_ref.py) against independent facts -- the analytic box and sphere SDFs,
winding numbers of off-surface points on the three real YCB meshes, the reference's own fixture clouds and
pitch table -- and the host-side layers: load_obj's face forms and YCBVideoModels on a directory tree."""
import os

import numpy as np
import pytest

import meshsdf_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YCB = {2: "003_cracker_box", 3: "004_sugar_box", 9: "010_potted_meat_can"}


def _ycb(name):
    d = np.load(os.path.join(GOLDEN, f"ycb_mesh_{name}.npz"))
    return d["vertices"], d["faces"]


def test_box_mesh_equals_analytic_sdf():
    lo, hi = (-0.2, 0.1, 0.3), (0.5, 0.35, 0.4)
    v, f = R.box_mesh(lo, hi)
    p = np.random.RandomState(0).uniform(-0.6, 0.9, (3000, 3))
    r = R.signed_distance(v, f, p)
    np.testing.assert_allclose(r["sdf"], R.box_sdf(p, lo, hi), rtol=0, atol=1e-12)
    assert set(np.round(r["winding"], 9)) <= {0.0, 1.0}


def test_icosphere_within_tessellation_bound():
    v, f = R.icosphere(3, 0.3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    r_in = np.min(np.abs(np.einsum("ij,ij->i", n / np.linalg.norm(n, axis=1)[:, None], a)))
    p = np.random.RandomState(1).uniform(-0.5, 0.5, (1500, 3))
    r = R.signed_distance(v, f, p)
    err = np.abs(r["sdf"] - (0.3 - np.linalg.norm(p, axis=1)))
    assert err.max() <= 0.3 - r_in + 1e-12
    clear = np.abs(np.linalg.norm(p, axis=1) - 0.3) > 0.3 - r_in  # not between the inscribed and the true sphere
    assert clear.sum() > 1000
    assert np.array_equal(r["winding"][clear] >= 0.5, np.linalg.norm(p[clear], axis=1) < 0.3)


@pytest.mark.parametrize("name", sorted(YCB.values()))
def test_ycb_winding_is_integral_off_surface(name):
    v, f = _ycb(name)
    lo, hi = v.min(0), v.max(0)
    p = np.random.RandomState(2).uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (400, 3))
    r = R.signed_distance(v, f, p, workers=4)
    off = r["dist"] > 1e-3
    assert off.sum() > 300
    w = r["winding"][off]
    assert np.all(np.minimum(np.abs(w), np.abs(w - 1.0)) < 1e-9)
    assert 0 < (w > 0.5).sum() < off.sum()


@pytest.mark.parametrize("fixture", [0, 1, 2])
def test_fixture_cloud_inside_its_mesh(fixture):
    d = np.load(os.path.join(GOLDEN, f"fixture_pose_refinement_0000000{fixture}.npz"))
    v, f = _ycb(YCB[int(d["class_id"])])
    r = R.signed_distance(v, f, d["pcd_cad"].astype(np.float64), workers=4)
    assert (r["sdf"] > 0).mean() >= 0.90


@pytest.mark.parametrize("class_id", sorted(YCB))
def test_pitch_from_mesh_matches_table(class_id):
    from morefusion_amd.synthetic import CLASS_PITCH
    v, _ = _ycb(YCB[class_id])
    ext = v.max(0) - v.min(0)
    pitch = np.sqrt((ext ** 2).sum()) / 32
    assert abs(pitch / CLASS_PITCH[class_id] - 1) <= 0.003


def test_load_obj_face_forms(tmp_path):
    from morefusion_amd.geometry import load_obj
    obj = tmp_path / "m.obj"
    obj.write_text("# comment\no thing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
                   "f 1 2 3\nf 1/1 3/1 4/1\nf 1//1 2//1 4//1\nf 2/1/1 3/1/1 4/1/1\nv 0 0 1\n"
                   "f -5 -4 -3 -1\ns off\nusemtl x\n")
    v, f = load_obj(obj)
    assert v.dtype == np.float64 and v.shape == (5, 3) and f.dtype == np.int32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3], [0, 1, 2], [0, 2, 4]]
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        load_obj(bad)


def _tree(root):
    v, f = R.box_mesh((0, 0, 0), (0.1, 0.2, 0.05))
    text = "".join(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in v)
    text += "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)
    for name, fname in (("002_a", "textured.obj"), ("010_b", "textured_simple.obj"), ("005_c", "textured.obj")):
        (root / name).mkdir()
        (root / name / fname).write_text(text)
    (root / "010_b" / "textured.obj").write_text("v 0 0 0\n")
    (root / "notes").mkdir()
    (root / "readme.txt").write_text("x")
    return v, f


def test_ycb_video_models_tree(tmp_path):
    from morefusion_amd.contrib.singleview_3d.models.model import Model
    from morefusion_amd.datasets import YCBVideoModels
    with pytest.raises(FileNotFoundError, match="NNN_name"):
        YCBVideoModels(tmp_path / "missing")
    v, f = _tree(tmp_path)
    m = YCBVideoModels(tmp_path)
    assert m.class_names == ["__background__", "002_a", "005_c", "010_b"]
    assert m.get_cad_file(3).name == "textured_simple.obj" and m.get_cad_file(1).name == "textured.obj"
    cad = m.get_cad(2)
    assert np.array_equal(cad.vertices, v) and np.array_equal(cad.faces, f)
    assert m.get_bbox_diagonal(1) == pytest.approx(np.sqrt(0.1 ** 2 + 0.2 ** 2 + 0.05 ** 2), rel=1e-15)
    assert m.get_voxel_pitch(32, 1) == m.get_bbox_diagonal(1) / 32
    assert m.get_pcd_file(1) == tmp_path / "002_a" / "points.xyz"
    with pytest.raises(FileNotFoundError):
        m.get_pcd(1)
    np.savetxt(tmp_path / "002_a" / "points.xyz", v)
    assert np.array_equal(m.get_pcd(1), v)
    with pytest.raises(IndexError):
        m.get_cad(4)
    # sdf.npz written by either side loads unchanged (the reference's keys)
    pts = np.random.RandomState(0).uniform(0, 0.05, (7, 3))
    sdf = np.arange(7, dtype=np.float64)
    np.savez_compressed(tmp_path / "005_c" / "sdf.npz", points=pts, sdf=sdf)
    got = m.get_sdf(2)
    assert np.array_equal(got[0], pts) and np.array_equal(got[1], sdf)
    assert m.get_sdf_batch([2, 2])[1][1] is got[1]
    # Model(models=...) takes it for its per-class pitch
    model = Model(n_fg_class=3, models=m)
    assert model._models.get_voxel_pitch(32, 1) == m.get_voxel_pitch(32, 1)


def test_morefusion_alias_resolves_datasets():
    import morefusion
    import morefusion_amd
    assert morefusion.datasets.YCBVideoModels is morefusion_amd.datasets.YCBVideoModels
    assert morefusion.geometry.mesh_signed_distance is morefusion_amd.geometry.mesh_signed_distance
