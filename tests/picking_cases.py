"""TEST INFRASTRUCTURE: the picking-order checks shared by tests/test_emul_picking.py (host emulator, 96 x 128) and
tests/test_gpu_picking.py (MI355X, 480 x 640).  Every check takes the device and the image size; bounds and cases
are the same on both.  The mirror is tests/picking_ref.py."""
import os
import warnings

import numpy as np
import pytest
import torch

import meshsdf_ref as R
import picking_ref as PR
import render_cases as C
import morefusion_amd as mf
from morefusion_amd.geometry.estimate_pointcloud_normals import _normals
from morefusion_amd.synthetic import _euler_pose

GOLDEN = os.path.join(C.GOLDEN, "ref_pointcloud_normals.npz")
GOLDEN_NAMES = ("plane", "sphere_cap", "plane_nan_step")
INTS = ("whole", "occluded_by", "bbox", "cell")
FLOATS = ("translation", "normal")


def same_bits(got, ref, what=""):
    """float64 arrays: NaN in the same places, every other element equal bit for bit."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    diff = got[~nan].view(np.int64) != ref[~nan].view(np.int64)
    assert not diff.any(), (what, int(diff.sum()))


def rotate(q, v):
    """v rotated by the unit quaternion q = (w, x, y, z)."""
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return Rm @ np.asarray(v, np.float64)


def same_analysis(got, ref):
    for k in INTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in FLOATS:
        same_bits(got[k], ref[k], k)


def ycb_scene():
    """Four YCB items (the cracker box twice) posed so that they overlap in the image: meshes, mesh_index, Ts, ids."""
    meshes = [C.ycb(2), C.ycb(3), C.ycb(9)]
    Ts = np.stack([_euler_pose(np.array(a), np.array(t)) for a, t in (
        ((1.0, 0.4, 2.0), (0.1, 0.0, 0.55)), ((0.2, 1.1, 0.7), (-0.02, -0.05, 0.7)),
        ((2.0, 0.1, 0.4), (0.05, 0.08, 0.45)), ((0.3, 0.5, 0.2), (-0.1, 0.02, 0.62)))])
    return meshes, [0, 1, 2, 0], Ts, [7, 3, 11, 5]


def check_bitwise(dev, H, W):
    K = C.intrinsics(H, W)
    meshes, index, Ts, ids = ycb_scene()
    got = mf.contrib.occlusion_analysis(meshes, Ts, K, H, W, instance_ids=ids, mesh_index=index, device=dev)
    ref = PR.analysis(meshes, Ts, K, H, W, ids, index)
    same_analysis(got, ref)
    assert np.array_equal(got["instance"].cpu().numpy(), ref["instance"][0])
    n = len(ids)
    off = got["occluded_by"][~np.eye(n, dtype=bool)]
    assert (got["whole"] > 0).all() and (off > 0).sum() >= 2 and (got["cell"] >= 0).all()  # they do occlude each other
    assert np.array_equal(got["occluded_by"].sum(axis=1), got["whole"])
    assert not np.isnan(got["translation"]).any() and not np.isnan(got["normal"]).any()
    with np.errstate(invalid="ignore"):
        expect = np.where(np.eye(n, dtype=bool), 0.0, got["occluded_by"] / got["whole"][:, None].astype(np.float64))
    assert np.array_equal(got["ratio"], expect)
    for k in range(n):
        same_bits(got["quaternion"][k], mf.contrib.quaternion_from_two_vectors([0, 0, 1], got["normal"][k]))
    # the items permuted: identical after un-permuting
    perm = [2, 0, 3, 1]
    again = mf.contrib.occlusion_analysis(meshes, Ts[perm], K, H, W, instance_ids=[ids[p] for p in perm],
                                          mesh_index=[index[p] for p in perm], device=dev)
    inv = np.argsort(perm)
    assert np.array_equal(again["instance"].cpu().numpy(), ref["instance"][0])
    back = {k: again[k][inv] for k in INTS + FLOATS}
    back["occluded_by"] = back["occluded_by"][:, inv]
    same_analysis(back, ref)


def _kernel_normals(points, dev, rect=None):
    pts = torch.as_tensor(np.ascontiguousarray(points)).to(dev)
    if rect is None:
        return mf.geometry.estimate_pointcloud_normals(pts).cpu().numpy()
    return _normals(pts[None], [rect])[0].cpu().numpy()


def check_normals(dev, H, W):
    gold = np.load(GOLDEN)
    for name in GOLDEN_NAMES:
        points, recorded = gold[f"points_{name}"], gold[f"normals_{name}"]
        assert points.shape == (24, 32, 3) and points.dtype == np.float64
        same_bits(PR.normals(points), recorded, f"mirror vs the reference's output, {name}")
        same_bits(_kernel_normals(points, dev), recorded, f"kernel vs the reference's output, {name}")
    assert np.isnan(gold["normals_plane_nan_step"]).any() and not np.isnan(gold["normals_plane"]).any()
    # a rendered depth image, back-projected in float64
    K = C.intrinsics(H, W)
    meshes, index, Ts, ids = ycb_scene()
    depth = mf.geometry.render_meshes(meshes, Ts, K, H, W, mesh_index=index, device=dev)["depth"][0].cpu().numpy()
    pcd = mf.geometry.pointcloud_from_depth(depth, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    assert pcd.dtype == np.float64
    ref = PR.normals(pcd)
    got = mf.geometry.estimate_pointcloud_normals(pcd, device=dev)
    assert got.dtype == torch.float64 and got.device.type == torch.device(dev).type
    same_bits(got.cpu().numpy(), ref, "rendered depth")
    assert (~np.isnan(ref).any(axis=2)).sum() > 200
    # float32 input is widened exactly
    same_bits(mf.geometry.estimate_pointcloud_normals(pcd.astype(np.float32), device=dev).cpu().numpy(),
              PR.normals(pcd.astype(np.float32).astype(np.float64)), "float32 input")
    # rectangle semantics: the normals of a sub-rectangle are the normals of the cropped array
    rect = (H // 4 + 1, W // 4 + 3, H - H // 4, W - W // 4 - 2)
    y1, x1, y2, x2 = rect
    sub = _kernel_normals(pcd, dev, rect)
    inside = np.zeros((H, W), bool)
    inside[y1:y2, x1:x2] = True
    assert np.isnan(sub[~inside]).all()
    crop = np.ascontiguousarray(pcd[y1:y2, x1:x2])
    same_bits(sub[y1:y2, x1:x2], _kernel_normals(crop, dev), "sub-rectangle vs crop (kernel)")
    same_bits(sub, PR.normals(pcd, rect), "sub-rectangle (mirror)")
    same_bits(PR.normals(pcd, rect)[y1:y2, x1:x2], PR.normals(crop), "sub-rectangle vs crop (mirror)")
    assert (~np.isnan(sub[y1:y2, x1:x2]).any(axis=2)).sum() > 100
    # the reference's argument checks
    with pytest.raises(NotImplementedError, match="KD-tree"):
        mf.geometry.estimate_pointcloud_normals(np.zeros((5, 3)))
    for shape in ((3,), (2, 2, 2, 3)):
        with pytest.raises(ValueError, match=r"\(H, W, 3\) or \(N, 3\)"):
            mf.geometry.estimate_pointcloud_normals(np.zeros(shape))


def check_plane_normals(dev, H, W):
    """z = a x + b y + c back-projected in float64: every interior normal parallel to (a, b, -1) within 1e-9."""
    K = C.intrinsics(H, W)
    a, b, c = 0.31, -0.22, 0.64
    i, j = np.mgrid[:H, :W].astype(np.float64)
    rx, ry = (j - K[0, 2]) / K[0, 0], (i - K[1, 2]) / K[1, 1]
    z = c / (1.0 - a * rx - b * ry)
    points = np.stack([rx * z, ry * z, z], -1)
    assert np.abs(a * points[..., 0] + b * points[..., 1] + c - z).max() < 1e-14 and z.min() > 0.3
    got = _kernel_normals(points, dev)
    assert not np.isnan(got).any()  # the border pixels too: one complete pair each
    want = np.array([a, b, -1.0]) / np.linalg.norm([a, b, -1.0])
    interior = got[2:-2, 2:-2]
    err = np.minimum(np.abs(interior - want).max(axis=-1), np.abs(interior + want).max(axis=-1))
    print(f"plane normals {H}x{W}: worst |n -+ (a, b, -1) / norm| = {err.max():.3e} (bound 1e-9)")
    assert err.max() <= 1e-9


def _slab(K, z, rows, cols, thick=1e-4):
    """A thin box whose front face, at depth z, covers exactly the pixel rows [rows) and columns [cols): its edges
    project onto half-integer pixel coordinates."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x0, x1 = ((c - 0.5 - cx) * z / fx for c in cols)
    y0, y1 = ((r - 0.5 - cy) * z / fy for r in rows)
    return R.box_mesh((x0, y0, z), (x1, y1, z + thick))


def check_known_answers(dev, H, W):
    """Three thin boxes on the axis at z = 1.0, 0.8, 0.6, each nearer one over the left half of the one behind; a
    small box over under 4 % of the farthest; a box fully hidden behind the farthest."""
    assert W % 64 == 0 and H * 4 == W * 3
    u = W // 32  # the image is 24 u x 32 u
    K = C.intrinsics(H, W)
    FAR, MID, NEAR, SMALL, HIDDEN = 10, 11, 12, 13, 14
    spans = {FAR: (1.0, (8 * u, 16 * u), (10 * u, 20 * u)), MID: (0.8, (7 * u, 17 * u), (5 * u, 15 * u)),
             NEAR: (0.6, (6 * u, 18 * u), (u, 10 * u)), SMALL: (0.5, (10 * u, 13 * u), (19 * u, 20 * u)),
             HIDDEN: (1.2, (10 * u, 12 * u), (16 * u, 18 * u))}
    ids = [FAR, MID, NEAR, SMALL, HIDDEN]
    classes = {FAR: 1, MID: 2, NEAR: 3, SMALL: 4, HIDDEN: 5}
    models = {classes[i]: _slab(K, *spans[i]) for i in ids}
    Ts = np.stack([np.eye(4)] * len(ids))
    picker = mf.contrib.SelectPickingOrder(models, target_class_id=classes[FAR], min_ratio=0.1, device=dev)
    res = picker([classes[i] for i in ids], ids, Ts, K, H, W)
    an = res["analysis"]
    k = {i: ids.index(i) for i in ids}
    for i in ids:  # every box alone covers exactly its rows x columns
        z, (r0, r1), (c0, c1) = spans[i]
        assert an["whole"][k[i]] == (r1 - r0) * (c1 - c0) and tuple(an["bbox"][k[i]]) == (r0, c0, r1, c1)
    cols_far, cols_mid = 10 * u, 10 * u
    assert abs(an["ratio"][k[FAR], k[MID]] - 0.5) <= 1.0 / cols_far
    assert abs(an["ratio"][k[MID], k[NEAR]] - 0.5) <= 1.0 / cols_mid
    assert an["ratio"][k[FAR], k[NEAR]] == 0.0 and an["ratio"][k[NEAR]].max() == 0.0
    assert 0.0 < an["ratio"][k[FAR], k[SMALL]] < 0.1  # seen, but no edge
    assert an["ratio"][k[HIDDEN], k[FAR]] == 1.0 and an["occluded_by"][k[HIDDEN], k[HIDDEN]] == 0
    assert set(res["edges"]) == {(FAR, MID), (MID, NEAR)}
    assert res["edges"][(FAR, MID)] == an["occluded_by"][k[FAR], k[MID]]
    assert res["order"] == [NEAR, MID, FAR]
    assert set(res["translation"]) == set(res["quaternion"]) == {FAR, MID, NEAR, SMALL}  # the hidden box: no node
    # grasp poses: a fronto-parallel face
    for i in ids:
        z, (r0, r1), (c0, c1) = spans[i]
        n, t, cell = an["normal"][k[i]], an["translation"][k[i]], int(an["cell"][k[i]])
        assert np.abs(np.abs(n) - (0.0, 0.0, 1.0)).max() <= 1e-12, (i, n)
        h, w = r1 - r0, c1 - c0
        S = max(1, int(np.floor(np.sqrt((h * w) // 30))))
        gw = -(-w // S)
        assert 0 <= cell < gw * -(-h // S)
        cr0, cc0 = r0 + (cell // gw) * S, c0 + (cell % gw) * S
        cr1, cc1 = min(cr0 + S, r1), min(cc0 + S, c1)
        zf = float(np.float32(z))
        centre = np.array([zf * ((cc0 + cc1 - 1) / 2 - K[0, 2]) / K[0, 0], zf * ((cr0 + cr1 - 1) / 2 - K[1, 2]) / K[1, 1], zf])
        half = 0.5 * zf / min(K[0, 0], K[1, 1])
        assert np.abs(t - centre).max() <= half, (i, t, centre)
        assert abs(t[2] - zf) <= 1e-6 * zf
        # the chosen cell is a central one: its centre within one cell of the box's centre
        assert abs((cr0 + cr1 - 1) / 2 - (r0 + r1 - 1) / 2) <= S and abs((cc0 + cc1 - 1) / 2 - (c0 + c1 - 1) / 2) <= S
        q = an["quaternion"][k[i]]
        assert abs(np.linalg.norm(q) - 1.0) <= 1e-12 and np.abs(rotate(q, (0, 0, 1)) - n).max() <= 1e-12
    # a target class that is absent, and one whose only instance is hidden
    for target in (9, classes[HIDDEN]):
        none = mf.contrib.SelectPickingOrder(models, target_class_id=target, device=dev)(
            [classes[i] for i in ids], ids, Ts, K, H, W)
        assert none["order"] == [] and set(none["edges"]) == {(FAR, MID), (MID, NEAR)}


def check_edges(dev, H, W):
    K = C.intrinsics(H, W)
    box = R.box_mesh((-0.05, -0.04, -0.03), (0.05, 0.04, 0.03))
    seen = _euler_pose(np.array((0.3, 0.5, 0.2)), np.array((0.0, 0.0, 0.5)))
    behind = _euler_pose(np.array((0.3, 0.5, 0.2)), np.array((0.0, 0.0, -0.5)))
    off = _euler_pose(np.array((0.3, 0.5, 0.2)), np.array((3.0, 0.0, 0.5)))
    ids = [4, 8, 6]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no division warning
        got = mf.contrib.occlusion_analysis([box], np.stack([behind, seen, off]), K, H, W, instance_ids=ids,
                                            mesh_index=[0, 0, 0], device=dev)
    same_analysis(got, PR.analysis([box], np.stack([behind, seen, off]), K, H, W, ids, [0, 0, 0]))
    assert got["whole"].tolist()[0] == 0 and got["whole"][1] > 0 and got["whole"][2] == 0
    for k in (0, 2):
        assert got["bbox"][k].tolist() == [0, 0, 0, 0] and got["cell"][k] == -1
        assert np.isnan(got["translation"][k]).all() and np.isnan(got["normal"][k]).all()
        assert np.isnan(got["quaternion"][k]).all() and (got["ratio"][k] == 0).all()
    assert (got["ratio"] == 0).all() and got["occluded_by"][1, 1] == got["whole"][1]
    res = mf.contrib.SelectPickingOrder({1: box}, target_class_id=1, device=dev)([1, 1, 1], ids, np.stack(
        [behind, seen, off]), K, H, W)
    assert res["order"] == [8] and set(res["translation"]) == {8} and res["edges"] == {}
    # zero items
    none = mf.contrib.occlusion_analysis([], np.zeros((0, 4, 4)), K, H, W, device=dev)
    assert none["instance"].shape == (H, W) and bool((none["instance"] == -1).all())
    for key, shape in (("whole", (0,)), ("occluded_by", (0, 0)), ("bbox", (0, 4)), ("ratio", (0, 0)), ("cell", (0,)),
                       ("translation", (0, 3)), ("normal", (0, 3)), ("quaternion", (0, 4))):
        assert none[key].shape == shape, key
    assert mf.contrib.SelectPickingOrder({1: box}, 1, device=dev)([], [], np.zeros((0, 4, 4)), K, H, W)["order"] == []
    # duplicate or negative ids
    for bad in ([1, 1], [0, -1]):
        with pytest.raises(ValueError, match="distinct"):
            mf.contrib.occlusion_analysis([box], np.stack([seen, seen]), K, H, W, instance_ids=bad, mesh_index=[0, 0],
                                          device=dev)
    # a one-pixel mask: S = 1, a point, no normal
    h, w = H // 2, W // 2
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    z = 0.5
    dot = R.box_mesh(((w - 0.4 - cx) * z / fx, (h - 0.4 - cy) * z / fy, z), ((w + 0.4 - cx) * z / fx, (h + 0.4 - cy) * z / fy, z + 1e-4))
    one = mf.contrib.occlusion_analysis([dot], np.eye(4)[None], K, H, W, device=dev)
    same_analysis(one, PR.analysis([dot], np.eye(4)[None], K, H, W, [0]))
    assert one["whole"].tolist() == [1] and one["bbox"].tolist() == [[h, w, h + 1, w + 1]] and one["cell"].tolist() == [0]
    assert np.isnan(one["normal"]).all() and np.isnan(one["quaternion"]).all()
    zf = float(np.float32(z))
    assert np.allclose(one["translation"][0], [zf * (w - cx) / fx, zf * (h - cy) / fy, zf], rtol=0, atol=1e-12)


def check_max_objects(dev):
    """MF_PICK_MAX_OBJECTS overlapping boxes at 48 x 64 against the mirror; one more raises."""
    H, W = 48, 64
    K = C.intrinsics(H, W)
    n = mf.contrib.picking_order.MAX_OBJECTS
    assert n >= 64
    box = R.box_mesh((-0.03, -0.025, -0.02), (0.03, 0.025, 0.02))
    rs = np.random.RandomState(5)
    Ts = np.stack([_euler_pose(rs.uniform(-1, 1, 3), np.array((rs.uniform(-0.2, 0.2), rs.uniform(-0.15, 0.15),
                                                               rs.uniform(0.4, 0.9)))) for _ in range(n + 1)])
    ids = rs.permutation(200)[:n + 1].tolist()
    got = mf.contrib.occlusion_analysis([box], Ts[:n], K, H, W, instance_ids=ids[:n], mesh_index=[0] * n, device=dev)
    ref = PR.analysis([box], Ts[:n], K, H, W, ids[:n], [0] * n)
    same_analysis(got, ref)
    assert (got["whole"] > 0).sum() >= n - 4 and (got["occluded_by"][~np.eye(n, dtype=bool)] > 0).sum() >= n // 2
    assert np.array_equal(got["occluded_by"].sum(axis=1), got["whole"])
    with pytest.raises(ValueError, match="MF_PICK_MAX_OBJECTS"):
        mf.contrib.occlusion_analysis([box], Ts, K, H, W, instance_ids=ids, mesh_index=[0] * (n + 1), device=dev)
