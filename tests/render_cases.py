"""TEST INFRASTRUCTURE: the render / full-grid / dataset checks shared by tests/test_emul_render.py (host
emulator, small images), tests/test_gpu_render.py (MI355X, 480 x 640) and tests/test_dataset_examples.py.
Every check takes the device and the image size; bounds and cases are the same on both."""
import os

import numpy as np
import torch

import meshsdf_ref as R
import render_ref as RR
import morefusion_amd as mf
from morefusion_amd.synthetic import _euler_pose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YCB = {2: "003_cracker_box", 3: "004_sugar_box", 9: "010_potted_meat_can"}


def ycb(class_id):
    d = np.load(os.path.join(GOLDEN, f"ycb_mesh_{YCB[class_id]}.npz"))
    return d["vertices"], d["faces"]


def intrinsics(height, width):
    s = width / 640.0
    return np.array([[619.4 * s, 0, width / 2 - 0.3], [0, 618.9 * s, height / 2 + 0.7], [0, 0, 1]])


def same(got, ref):
    """depth (as bits), instance, face, count: equal."""
    for k in ("depth", "instance", "face", "count"):
        g, r = got[k].cpu().numpy(), ref[k]
        assert g.dtype == r.dtype and g.shape == r.shape, (k, g.dtype, r.dtype, g.shape, r.shape)
        if k == "depth":
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert np.array_equal(g, r), (k, int((g != r).sum()))


def scene():
    """Box, icosphere and the three YCB meshes, posed so that they occlude each other in one image."""
    meshes = [R.box_mesh((-0.1, -0.1, -0.1), (0.1, 0.12, 0.15)), R.icosphere(2, 0.1), ycb(2), ycb(3), ycb(9)]
    Ts = [_euler_pose(np.array(a), np.array(t)) for a, t in (
        ((0.3, 0.5, 0.2), (-0.12, 0.0, 0.62)), ((0, 0, 0), (0.0, 0.03, 0.5)), ((1.0, 0.4, 2.0), (0.1, 0.0, 0.55)),
        ((0.2, 1.1, 0.7), (-0.02, -0.05, 0.7)), ((2.0, 0.1, 0.4), (0.05, 0.08, 0.45)))]
    return meshes, np.stack(Ts)


def check_bitwise(dev, H, W):
    K = intrinsics(H, W)
    meshes, Ts = scene()
    n = len(meshes)
    ids = [7, 3, 11, 5, 2]
    # every mesh in an image of its own (what render_cad draws) and the composite, one launch each
    same(mf.geometry.render_meshes(meshes, Ts, K, H, W, targets=range(n), instance_ids=ids, device=dev),
         RR.render(meshes, Ts, K, H, W, targets=range(n), instance_ids=ids))
    comp = mf.geometry.render_meshes(meshes, Ts, K, H, W, instance_ids=ids, device=dev)
    ref = RR.render(meshes, Ts, K, H, W, instance_ids=ids)
    same(comp, ref)
    assert (ref["count"] > 0).all() and len(np.unique(ref["instance"])) == n + 1  # all visible, background too
    alone = RR.render(meshes, Ts, K, H, W, targets=range(n))["count"]
    assert (ref["count"] < alone).sum() >= 2  # mutual occlusion
    # order independence: the faces of every mesh permuted, the face ids mapped back
    rs = np.random.RandomState(0)
    perms = [rs.permutation(len(f)) for _, f in meshes]
    shuffled = [(v, np.asarray(f)[p]) for (v, f), p in zip(meshes, perms)]
    got = mf.geometry.render_meshes(shuffled, Ts, K, H, W, instance_ids=ids, device=dev)
    assert np.array_equal(got["depth"].cpu().numpy().view(np.uint32), ref["depth"].view(np.uint32))
    assert np.array_equal(got["instance"].cpu().numpy(), ref["instance"])
    assert np.array_equal(got["count"].cpu().numpy(), ref["count"])
    face, inst = got["face"].cpu().numpy(), ref["instance"]
    back = np.full(face.shape, -1, np.int32)
    for k, p in enumerate(perms):
        m = inst == ids[k]
        back[m] = p[face[m]]
    assert np.array_equal(back, ref["face"])


def check_edge_cases(dev, H, W):
    K = intrinsics(H, W)
    box = R.box_mesh((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1))
    # partly outside the image; a box reaching behind the near plane (faces with a vertex at z <= near dropped whole)
    for T in (_euler_pose(np.array((0.2, 0.3, 0.1)), np.array((0.32, -0.2, 0.55))),
              _euler_pose(np.array((0.4, 0.2, 0.0)), np.array((0.02, 0.01, 0.1)))):
        ref = RR.render([box], [T], K, H, W)
        same(mf.geometry.render_meshes([box], [T], K, H, W, device=dev), ref)
        assert 0 < ref["count"][0] < H * W
    rec = RR.setup(*box, T, K, H, W)
    v_cam = box[0] @ T[:3, :3].T + T[:3, 3]
    behind = (v_cam[:, 2] <= 0.01)[box[1]].any(axis=1)
    assert behind.any() and not behind.all() and not rec["valid"][behind].any()
    # degenerate faces: a repeated vertex, three collinear vertices, one point, an index outside the mesh
    bv = np.vstack([box[0], [[0.0, 0.0, 0.3], [0.0, 0.05, 0.3], [0.0, 0.1, 0.3]]])
    bf = np.vstack([box[1], [[8, 8, 9], [8, 9, 10], [10, 10, 10], [0, 1, 99]]]).astype(np.int32)
    T = _euler_pose(np.array((0.3, 0.5, 0.2)), np.array((0.0, 0.0, 0.6)))
    ref = RR.render([(bv, bf)], [T], K, H, W)
    same(mf.geometry.render_meshes([(bv, bf)], [T], K, H, W, device=dev), ref)
    assert ref["face"].max() < 12 and np.array_equal(ref["depth"].view(np.uint32),
                                                     RR.render([box], [T], K, H, W)["depth"].view(np.uint32))
    # an empty item list: one empty image
    got = mf.geometry.render_meshes([], np.zeros((0, 4, 4)), K, H, W, device=dev)
    assert got["depth"].shape == (1, H, W) and bool(torch.isnan(got["depth"]).all())
    assert bool((got["instance"] == -1).all()) and bool((got["face"] == -1).all()) and got["count"].shape == (0,)


def _rays(K, H, W):
    i, j = np.mgrid[:H, :W].astype(np.float64)
    return np.stack([(j - K[0, 2]) / K[0, 0], (i - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)


def _edge_clearance(corners_uv, edges, H, W):
    """Smallest distance (pixels) from a pixel centre to a projected edge segment."""
    i, j = np.mgrid[:H, :W].astype(np.float64)
    best = np.inf
    for a, b in edges:
        p, q = corners_uv[a], corners_uv[b]
        d = q - p
        t = np.clip(((j - p[0]) * d[0] + (i - p[1]) * d[1]) / (d @ d), 0.0, 1.0)
        best = min(best, float(np.hypot(j - (p[0] + t * d[0]), i - (p[1] + t * d[1])).min()))
    return best


def check_box_analytic(dev, H, W):
    """Mask exactly the analytic ray-box intersection, |depth - analytic| <= 2^-22 depth.  Returns the worst
    |depth - analytic| / depth."""
    K = intrinsics(H, W)
    lo, hi = np.array((-0.11, -0.07, -0.09)), np.array((0.13, 0.1, 0.06))
    worst = 0.0
    for ang, t in (((0.31, 0.52, 0.23), (-0.04, 0.02, 0.61)), ((1.2, -0.4, 2.1), (0.07, -0.03, 0.48))):
        T = _euler_pose(np.array(ang), np.array(t))
        Rm, tr = T[:3, :3], T[:3, 3]
        d = _rays(K, H, W) @ Rm  # the rays in the box frame: R^T d, origin -R^T t
        o = -Rm.T @ tr
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - o) / d, (hi - o) / d
        tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
        hit = (tn <= tf) & (tn > 0)
        corners = np.array([[(lo, hi)[x][0], (lo, hi)[y][1], (lo, hi)[z][2]] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
        cam = corners @ Rm.T + tr
        uv = np.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], 1)
        edges = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]
        assert len(edges) == 12 and _edge_clearance(uv, edges, H, W) > 1e-6  # a generic pose
        got = mf.geometry.render_meshes([R.box_mesh(lo, hi)], [T], K, H, W, device=dev)
        depth = got["depth"][0].cpu().numpy().astype(np.float64)
        assert np.array_equal(~np.isnan(depth), hit) and hit.sum() > 50
        ratio = float((np.abs(depth[hit] - tn[hit]) / depth[hit]).max())  # (the ray has unit z: t is the depth)
        print(f"box analytic {H}x{W}: {int(hit.sum())} px, worst |depth - analytic| / depth = {ratio:.3e} "
              f"(bound {2.0 ** -22:.3e})")
        assert ratio <= 2.0 ** -22
        worst = max(worst, ratio)
    return worst


def check_icosphere_analytic(dev, H, W):
    K = intrinsics(H, W)
    r = 0.1
    v, f = R.icosphere(3, r)
    c = np.array((0.03, -0.02, 0.5))
    T = _euler_pose(np.array((0.3, 0.2, 0.1)), c)
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    sag = r - float(np.abs((n * tri[:, 0]).sum(1)).min())
    assert 0 < sag < 0.01 * r
    got = mf.geometry.render_meshes([(v, f)], [T], K, H, W, device=dev)
    depth = got["depth"][0].cpu().numpy()
    covered = ~np.isnan(depth)
    d = _rays(K, H, W)
    dd, b = (d * d).sum(-1), d @ c

    def sphere(radius):
        disc = b * b - dd * (c @ c - radius * radius)
        with np.errstate(invalid="ignore"):
            return disc >= 0, (b - np.sqrt(disc)) / dd
    hit, z = sphere(r)
    with np.errstate(invalid="ignore"):
        p = d * z[..., None]
        cosine = -((p - c) / r * d).sum(-1) / np.sqrt(dd)
        front = hit & (cosine >= 0.5)
    assert front.sum() > 50 and covered[front].all()
    diff = depth.astype(np.float64)[front] - z[front]
    print(f"icosphere {H}x{W}: sag {sag:.3e}, depth - sphere in [{diff.min():.3e}, {diff.max():.3e}]")
    assert (diff >= 0).all() and (diff <= 2 * sag).all()
    inner, _ = sphere(r - sag)  # a ray through the inscribed sphere meets the polyhedron around it
    border = np.zeros((H, W), bool)
    border[[0, -1]] = border[:, [0, -1]] = True
    assert inner.sum() > 50 and covered[inner & ~border].all()
    # the depth back-projected lies on the mesh
    pcd = mf.geometry.pointcloud_from_depth(depth, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pad = np.pad(covered, 1)
    interior = covered.copy()
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            interior &= pad[di:di + H, dj:dj + W]
    pts = (pcd[interior].astype(np.float64) - T[:3, 3]) @ T[:3, :3]  # to the mesh frame: R^T (p - t)
    sdf = mf.geometry.mesh_signed_distance(v, f, torch.as_tensor(pts).to(dev)).cpu().numpy()
    print(f"icosphere {H}x{W}: {int(interior.sum())} interior px, max |sdf| = {np.abs(sdf).max():.3e}")
    assert interior.sum() > 50 and np.abs(sdf).max() <= 1e-6


def check_render_cad(dev, H, W):
    fovy = 45.0
    K = mf.extra._render.fovy_intrinsics(fovy, H, W)
    assert K[0, 0] == K[1, 1] == (H / 2) / np.tan(np.radians(fovy) / 2) and K[0, 2] == W / 2 - 0.5 and K[1, 2] == H / 2 - 0.5
    cad = ycb(3)
    Ts = np.stack([_euler_pose(np.array(a), np.array(t)) for a, t in (
        ((0.3, 0.5, 0.2), (0.0, 0.0, 0.5)), ((1.0, 0.4, 2.0), (0.1, 0.0, 0.6)), ((2.0, 0.1, 0.4), (-0.05, 0.05, 0.45)))])
    rgb, depths, masks, counts = mf.extra.render_cad(cad, Ts, fovy, H, W, device=dev, return_count=True)
    assert rgb is None and depths.shape == (3, H, W) and depths.dtype == np.float32 and masks.dtype == bool
    assert np.array_equal(counts, masks.sum(axis=(1, 2))) and (counts > 0).all()
    assert np.array_equal(masks, ~np.isnan(depths))
    for k in range(3):
        none, d1, m1 = mf.extra.render_cad(cad, Ts[k], fovy, H, W, device=dev)
        assert none is None and d1.shape == (H, W)
        assert np.array_equal(d1.view(np.uint32), depths[k].view(np.uint32)) and np.array_equal(m1, masks[k])
    # alone in the frame: the label of its own composite is the render, visibility exactly 1
    comp = mf.geometry.render_meshes([cad], Ts[:1], K, H, W, instance_ids=[4], device=dev)
    mask = comp["instance"][0].cpu().numpy() == 4
    assert 1.0 * mask.sum() / counts[0] == 1.0
    # occluded by a nearer box: axis-aligned boxes on the optical axis, so the pixel counts are known.  The object's
    # silhouette is its front face (x in [-a, a], y in [-b, b] at z0); the occluder covers x >= x0 and its silhouette's
    # left border is the projection of its BACK face's edge (x0 > 0: farther is further left)
    fy, cx, cy = K[1, 1], K[0, 2], K[1, 2]
    a, b, z0, x0, zb = 0.0503, 0.0301, 0.4, 0.0107, 0.3
    obj = R.box_mesh((-a, -b, z0), (a, b, z0 + 0.05))
    occ = R.box_mesh((x0, -1.0, 0.25), (2.0, 1.0, zb))
    cols = np.arange(W)[np.abs(np.arange(W) - cx) < fy * a / z0]
    rows = np.arange(H)[np.abs(np.arange(H) - cy) < fy * b / z0]
    seen = cols[cols - cx < fy * x0 / zb]
    for e in (fy * a / z0, fy * b / z0, fy * x0 / zb):  # no pixel centre on a border
        assert min(np.abs(np.abs(np.arange(max(H, W)) - c) - e).min() for c in (cx, cy)) > 1e-6
    assert 0 < len(seen) < len(cols) and len(rows) > 0
    _, _, m_rend, n_rend = mf.extra.render_cad(obj, np.eye(4), fovy, H, W, device=dev, return_count=True)
    assert n_rend == len(cols) * len(rows) == m_rend.sum()
    comp = mf.geometry.render_meshes([obj, occ], np.stack([np.eye(4)] * 2), K, H, W, instance_ids=[4, 6], device=dev)
    mask = comp["instance"][0].cpu().numpy() == 4
    with np.errstate(invalid="ignore"):
        visibility = 1.0 * mask.sum() / m_rend.sum()
    assert visibility == (len(seen) * len(rows)) / (len(cols) * len(rows)) and 0 < visibility < 1


def grid_full_numpy(points, Ts, pitch, origin, dim=32):
    """The reference's _get_grid_full over a list of (points, T), restated: labels 1, 2, ... in list order, the
    last writer wins.  Also returns the smallest distance of a grid coordinate to a half-integer."""
    grid = np.zeros((dim,) * 3, np.int32)
    margin = np.inf
    for i, (p, T) in enumerate(zip(points, Ts)):
        q = (np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3] - origin) / pitch
        if q.size:
            margin = min(margin, float(np.abs(q - np.floor(q) - 0.5).min()))
        idx = np.round(q).astype(int)
        keep = ((idx >= 0) & (idx < dim)).all(axis=1)
        I, J, K = idx[keep].T
        grid[I, J, K] = i + 1
    return grid, margin


def check_full_grids(dev):
    rs = np.random.RandomState(3)
    n, dim = 3, 32
    # three solid blobs a few voxels apart, each grid centred on its own object: the grids overlap
    points = [rs.uniform(-0.04, 0.04, (4000, 3)) * np.array(s) for s in ((1, 1, 1), (1.2, 0.6, 0.8), (0.5, 1.3, 1))]
    Ts = np.stack([_euler_pose(rs.uniform(-1, 1, 3), np.array(t)) for t in ((0, 0, 0.6), (0.05, 0.01, 0.62), (0.02, 0.06, 0.58))])
    pitch = np.array([0.0061, 0.0053, 0.0068])
    origin = Ts[:, :3, 3] - 15.5 * pitch[:, None] + rs.uniform(-0.002, 0.002, (n, 3))

    def expect(points, Ts, pitch, origin):
        gt, gn, margin = [], [], np.inf
        for e in range(len(points)):
            others = [i for i in range(len(points)) if i != e]
            g, m1 = grid_full_numpy([points[e]], [Ts[e]], pitch[e], origin[e], dim)
            h, m2 = grid_full_numpy([points[i] for i in others], [Ts[i] for i in others], pitch[e], origin[e], dim)
            gt.append(g)
            gn.append(h)
            margin = min(margin, m1, m2)
        return np.stack(gt), np.stack(gn), margin
    gt, gn, margin = expect(points, Ts, pitch, origin)
    assert margin > 1e-6  # no coordinate near a rounding tie: no mismatch allowed
    got_t, got_n = mf.geometry.full_grids(points, Ts, pitch, origin, dim=dim, device=dev)
    assert got_t.dtype == torch.int32 and got_n.dtype == torch.int32
    assert np.array_equal(got_t.cpu().numpy(), gt) and np.array_equal(got_n.cpu().numpy(), gn)
    for e in range(n):  # the order of the labels matters: both labels present, and voxels two objects share
        assert set(np.unique(gn[e])) == {0, 1, 2} and gt[e].sum() > 100
    shared = ((grid_full_numpy([points[0]], [Ts[0]], pitch[2], origin[2])[0] > 0)
              & (grid_full_numpy([points[1]], [Ts[1]], pitch[2], origin[2])[0] > 0))
    assert shared.sum() > 0 and (gn[2][shared] == 2).all()  # the later of the two wins a shared voxel
    # one example alone: nothing else in its grid
    a_t, a_n = mf.geometry.full_grids(points[:1], Ts[:1], pitch[:1], origin[:1], device=dev)
    assert np.array_equal(a_t.cpu().numpy(), gt[:1]) and not bool(a_n.any())
    # points entirely outside every grid
    far = [p + 5.0 for p in points[:2]]
    f_t, f_n = mf.geometry.full_grids(far, np.stack([np.eye(4)] * 2), pitch[:2], origin[:2], device=dev)
    assert not bool(f_t.any()) and not bool(f_n.any())


class CadFrameDataset(mf.datasets.RGBDPoseEstimationDatasetBase):
    """Frames of synthetic.make_cad_frame over the three committed YCB meshes."""

    _shared = {}  # device -> the models adapter (its solid grids are voxelized once per test process)

    def __init__(self, H, W, device, class_ids=None, edit=None):
        self.meshes = {c: ycb(c) for c in YCB}
        if device not in self._shared:
            self._shared[device] = mf.datasets.as_models(self.meshes, device)
        super().__init__(self._shared[device], class_ids=class_ids, device=device)
        self.H, self.W, self.edit = H, W, edit
        if device == "cpu":  # the host emulator: a 32^3 solid grid (cells below the 32^3 target grid's pitch still)
            self._solid_dim = 32

    def get_frame(self, index):
        frame = mf.synthetic.make_cad_frame(self.meshes, seed=index, height=self.H, width=self.W, n_objects=3,
                                            device=self._device)
        return self.edit(frame) if self.edit else frame


KEYS = ("class_id", "rgb", "pcd", "quaternion_true", "translation_true", "visibility", "origin", "pitch",
        "grid_target", "grid_nontarget", "grid_empty", "grid_target_full", "grid_nontarget_full")


def check_examples(dev, H, W):
    """Schema, pose round trip, grid_target inside the dilated grid_target_full.  Returns (examples, frame, share)."""
    ds = CadFrameDataset(H, W, dev)
    frame = ds.get_frame(0)
    assert frame["depth"].shape == (H, W) and np.isnan(frame["depth"]).any() and frame["rgb"].dtype == np.uint8
    assert set(np.unique(frame["label"])) == {0, 1, 2, 3, 4}
    examples = ds.get_example(0)
    assert len(examples) == 3
    inside = total = 0
    for k, ex in enumerate(examples):
        assert tuple(ex) == KEYS
        assert ex["class_id"] == frame["class_ids"][k] and ex["class_id"].dtype == np.int32
        assert ex["rgb"].shape == (256, 256, 3) and ex["rgb"].dtype == np.uint8
        assert ex["pcd"].shape == (256, 256, 3) and ex["pcd"].dtype == np.float64
        assert ex["quaternion_true"].shape == (4,) and ex["translation_true"].shape == (3,)
        assert ex["quaternion_true"].dtype == ex["translation_true"].dtype == np.float64
        assert ex["origin"].shape == (3,) and ex["origin"].dtype == np.float64 and np.ndim(ex["pitch"]) == 0
        assert ex["pitch"] == ds._models.get_voxel_pitch(32, ex["class_id"])
        for g in ("grid_target", "grid_nontarget", "grid_empty"):
            assert ex[g].shape == (32, 32, 32) and ex[g].dtype == np.float32
        for g in ("grid_target_full", "grid_nontarget_full"):
            assert ex[g].shape == (32, 32, 32) and ex[g].dtype == np.int32
        assert set(np.unique(ex["grid_target_full"])) == {0, 1} and ex["grid_nontarget_full"].max() <= 2
        assert np.isfinite(ex["visibility"]) and 0.5 < ex["visibility"] <= 1.05
        # the pose round trip
        from morefusion_amd.datasets.rgbd_pose_estimation import _quaternion_matrix
        T = _quaternion_matrix(ex["quaternion_true"])
        T[:3, 3] = ex["translation_true"]
        np.testing.assert_allclose(T, frame["Ts_cad2cam"][k], rtol=0, atol=1e-12)
        # origin = nan-median of the crop - 15.5 pitch
        np.testing.assert_allclose(ex["origin"], np.nanmedian(ex["pcd"], axis=(0, 1)) - 15.5 * ex["pitch"], atol=1e-12)
        tgt = ex["grid_target"] > 0.5
        full = ex["grid_target_full"] > 0
        dil = np.pad(full, 1)
        dilated = np.zeros_like(full)
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    dilated |= dil[a:a + 32, b:b + 32, c:c + 32]
        assert tgt.sum() > 20
        inside += int((tgt & dilated).sum())
        total += int(tgt.sum())
    share = inside / total
    print(f"get_example {H}x{W}: grid_target inside dilated grid_target_full: {inside} / {total} = {share:.4f}")
    assert share >= 0.9
    return ds, examples, frame, share


def check_skips(dev, H, W):
    def edit(frame):  # object 0 becomes background class 0; an id without pixels is appended (empty box)
        frame = dict(frame)
        frame["class_ids"] = frame["class_ids"].copy()
        frame["class_ids"][0] = 0
        frame["instance_ids"] = np.append(frame["instance_ids"], 40).astype(np.int32)
        frame["class_ids"] = np.append(frame["class_ids"], 2).astype(np.int32)
        frame["Ts_cad2cam"] = np.concatenate([frame["Ts_cad2cam"], np.eye(4)[None]])
        return frame
    ds = CadFrameDataset(H, W, dev, edit=edit)
    frame = ds.get_frame(0)
    ex = ds.get_example(0)
    assert [e["class_id"] for e in ex] == frame["class_ids"][1:3].tolist()
    assert all(e["grid_nontarget_full"].max() <= 1 for e in ex)  # one other example each
    only = int(frame["class_ids"][2])
    ex = CadFrameDataset(H, W, dev, class_ids=[only], edit=edit).get_example(0)
    assert [int(e["class_id"]) for e in ex] == [only] and not ex[0]["grid_nontarget_full"].any()

    class Sparse(CadFrameDataset):
        _n_points_minimal = 10 ** 7
    assert Sparse(H, W, dev).get_example(0) == []

    def none(frame):
        return dict(frame, instance_ids=np.zeros(0, np.int32), class_ids=np.zeros(0, np.int32),
                    Ts_cad2cam=np.zeros((0, 4, 4)))
    assert CadFrameDataset(H, W, dev, edit=none).get_example(0) == []
