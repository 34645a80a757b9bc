"""TEST HELPER: the grids of tests/test_gridmesh_host.py, tests/test_emul_gridmesh.py and tests/test_gpu_gridmesh.py
-- the smallest shapes at which csrc/gridmesh.hip can go wrong -- and the comparisons the emulator and GPU tests share."""
import functools

import numpy as np

import gridmesh_ref as M
import occserver_cases as OC
import occtrack_cases as TC

RANDOM_SEED = 0


def one_voxel():
    g = np.zeros((3, 3, 3), np.float32)
    g[1, 1, 1] = 1
    return g


def diagonal_pair(step):
    """Two voxels that touch only along ``step``: (1,1,1) joins them in this subdivision, (1,-1,1) does not."""
    g = np.zeros((4, 4, 4), np.float32)
    a = np.array([1, 2 if step[1] < 0 else 1, 1])
    g[tuple(a)] = 0.7
    g[tuple(a + np.asarray(step))] = 0.9
    return g


def corners(dims=(4, 3, 5)):
    """Voxels in cells 0 and dim - 1 of every axis: only the padding closes the surface."""
    g = np.zeros(dims, np.float32)
    for i in (0, dims[0] - 1):
        for j in (0, dims[1] - 1):
            for k in (0, dims[2] - 1):
                g[i, j, k] = 1
    return g


def random_grid(seed=RANDOM_SEED):
    """5 x 7 x 6 at density 0.5; values on both sides of 0 (occupied iff > 0), one NaN (not occupied)."""
    rs = np.random.RandomState(seed)
    g = rs.uniform(-1, 1, (5, 7, 6)).astype(np.float32)
    g[0, 0, 0] = np.nan
    return g


def full():
    return np.full((32, 32, 32), 0.97, np.float32)


def checkerboard():
    i, j, k = np.indices((32, 32, 32))
    return ((i + j + k) % 2).astype(np.float32)


def blobs(seed, n=16):
    """Three different blobby 16^3 grids (union of balls), for the label test."""
    rs = np.random.RandomState(seed)
    x = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).astype(np.float64)
    g = np.zeros((n, n, n), np.float32)
    for _ in range(4):
        c, r = rs.uniform(4, n - 4, 3), rs.uniform(2.5, 4.5)
        g[((x - c) ** 2).sum(-1) < r * r] = 0.9
    return g


SMALL = dict(one_voxel=one_voxel, joined=lambda: diagonal_pair((1, 1, 1)), apart=lambda: diagonal_pair((1, -1, 1)),
             corners=corners, random=random_grid)


@functools.lru_cache(maxsize=None)
def small_batch():
    """The small grids as one ragged batch -> (grids, pitch, origin, mirror meshes unsmoothed)."""
    grids = [SMALL[k]() for k in SMALL]
    pitch = np.array([0.01, 0.004375644727606043, 0.5, 1.0, 0.0078125][:len(grids)], np.float32)
    origin = np.array([[0.1 * b, -0.3, 0.25 + b] for b in range(len(grids))], np.float64)
    ref = [M.mesh(g, h, o) for g, h, o in zip(grids, pitch, origin)]
    return grids, pitch, origin, ref


@functools.lru_cache(maxsize=None)
def big_batch():
    """An empty grid, a 1 x 1 x 1 grid, a full 32^3 and the 32^3 checkerboard (the vertex maximum)."""
    grids = [np.zeros((2, 3, 2), np.float32), np.ones((1, 1, 1), np.float32), full(), checkerboard()]
    pitch = np.array([0.01, 0.02, 0.005, 0.01], np.float32)
    origin = np.array([[0, 0, 0], [1, 2, 3], [-0.1, 0.2, 0.6], [0.3, 0.3, 0.3]], np.float64)
    ref = [M.mesh(g, h, o) for g, h, o in zip(grids, pitch, origin)]
    return grids, pitch, origin, ref


def to_numpy(meshes):
    return [(v.cpu().numpy(), f.cpu().numpy()) for v, f in meshes]


def assert_meshes_equal(got, exp):
    assert len(got) == len(exp)
    for b, ((v, f), (ve, fe)) in enumerate(zip(got, exp)):
        assert v.dtype == np.float64 and f.dtype == np.int32, b
        assert v.shape == ve.shape and f.shape == fe.shape, (b, v.shape, ve.shape, f.shape, fe.shape)
        assert np.array_equal(f, fe), b
        assert np.array_equal(v, ve), (b, float(np.abs(v - ve).max()) if len(v) else 0.0)


def check_extraction(batch, device):
    """Vertices, faces and offsets of the product equal the mirror's, unsmoothed and with iterations=0."""
    from morefusion_amd.geometry import grid_mesh
    grids, pitch, origin, ref = batch
    plan = grid_mesh.GridMeshPlan(grids, pitch, origin, device=device)
    plan.count()
    assert plan.v_off == np.concatenate([[0], np.cumsum([len(v) for v, _ in ref])]).tolist()
    assert plan.f_off == np.concatenate([[0], np.cumsum([len(f) for _, f in ref])]).tolist()
    plan.emit()
    assert_meshes_equal(to_numpy(plan.meshes()), ref)
    got = grid_mesh.voxel_grids_to_meshes(grids, pitch, origin, iterations=0, device=device)
    assert_meshes_equal(to_numpy(got), ref)
    return plan


def check_smoothing(batch, device, iterations):
    from morefusion_amd.geometry import grid_mesh
    grids, pitch, origin, ref = batch
    got = to_numpy(grid_mesh.voxel_grids_to_meshes(grids, pitch, origin, iterations=iterations, device=device))
    exp = [(M.humphrey(v, f, iterations=iterations), f) for v, f in ref]
    assert_meshes_equal(got, exp)
    if iterations:
        assert any(len(v) and not np.array_equal(v, ve) for (v, _), (ve, _) in zip(got, ref))  # it moved something


# ---- the label test: three meshes from 16^3 grids in a 48 x 64 image ------------------------------------------------
LABEL_H, LABEL_W = 48, 64
LABEL_K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])


@functools.lru_cache(maxsize=None)
def label_scene():
    """-> (grids dict in the map frame, sensor depth [48, 64] float32, T_sensor_to_map, mirror label, branch counts)."""
    pitch = np.array([0.02, 0.015, 0.02], np.float32)
    centre = np.array([[-0.25, 0.0, 1.0], [0.05, 0.05, 0.9], [0.3, -0.05, 1.1]])
    c, s = np.cos(0.2), np.sin(0.2)
    T = np.array([[c, 0, s, 0.1], [0, 1, 0, -0.05], [-s, 0, c, 0.02], [0, 0, 0, 1]], np.float64)  # sensor -> map
    origin = (T[:3, :3] @ centre.T).T + T[:3, 3] - 7.5 * pitch[:, None].astype(np.float64)
    grids = dict(instance_ids=[3, 5, 8], class_ids=[1, 2, 3], pitch=pitch, origin=origin,
                 grid=np.stack([blobs(s) for s in (1, 2, 3)]))
    # the sensor depth: the render's own depth shifted by -3 cm .. +3 cm in vertical bands (both sides of the 1 cm
    # margin), the table plane behind where nothing is drawn, NaN in a diagonal stripe
    _, _, parts = M.render_voxel_grids(grids, np.zeros((LABEL_H, LABEL_W), np.float32), LABEL_K, T, LABEL_H, LABEL_W,
                                       return_parts=True)
    jj, ii = np.indices((LABEL_H, LABEL_W))
    shift = (np.array([-0.03, -0.012, -0.008, 0.0, 0.008, 0.03], np.float32))[(ii // 3) % 6]
    depth = np.where(np.isnan(parts["depth"][0]), np.float32(1.5), parts["depth"][0] + shift).astype(np.float32)
    depth[(ii + jj) % 7 == 0] = np.nan
    label, counts, _ = M.render_voxel_grids(grids, depth, LABEL_K, T, LABEL_H, LABEL_W, return_parts=True)
    return grids, depth, T, label, counts


def check_label(device):
    import torch
    from morefusion_amd.contrib import render_voxel_grids
    grids, depth, T, label, _ = label_scene()
    g = dict(grids, **{k: torch.from_numpy(np.ascontiguousarray(grids[k])).to(device) for k in ("pitch", "origin", "grid")})
    got = render_voxel_grids(g, torch.from_numpy(depth).to(device), LABEL_K, T, LABEL_H, LABEL_W)
    assert got.dtype == torch.int32 and tuple(got.shape) == (LABEL_H, LABEL_W)
    assert np.array_equal(got.cpu().numpy(), label)
    empty = dict(g, grid=torch.zeros_like(g["grid"]))
    assert (render_voxel_grids(empty, torch.from_numpy(depth).to(device), LABEL_K, T, LABEL_H, LABEL_W) == -2).all()
    none = dict(instance_ids=[], class_ids=[], pitch=g["pitch"][:0], origin=g["origin"][:0], grid=g["grid"][:0])
    assert (render_voxel_grids(none, torch.from_numpy(depth).to(device), LABEL_K, T, LABEL_H, LABEL_W) == -2).all()


# ---- the map-frame grids and the tracker's two render routes on the scene of occserver_cases.make_frames -----------
def check_map_grids(server, ref):
    got, exp = server.grids_in_map_frame(), M.grids_in_map_frame(ref)
    assert got["instance_ids"] == exp["instance_ids"] and got["class_ids"] == exp["class_ids"] and len(exp["instance_ids"]) >= 3
    for k, dtype in (("pitch", np.float32), ("origin", np.float64), ("grid", np.float32)):
        g = got[k].cpu().numpy()
        assert g.dtype == dtype and g.shape == exp[k].shape and np.array_equal(g, exp[k]), k
    for b, i in enumerate(exp["instance_ids"]):
        assert np.array_equal(exp["origin"][b], ref.centers[i].astype(np.float64) - 15.5 * np.float64(exp["pitch"][b]))
    occupied = (exp["grid"] > 0).reshape(len(exp["instance_ids"]), -1).sum(axis=1)
    assert (occupied > 0).all() and (exp["grid"][exp["grid"] > 0] > 0.5).all()
    return got


def thresholds(height):
    """The synthetic objects are 30 .. 100 pixels across at 480 rows: the vetoes examples/online_pose_refinement.py uses
    for them (20 / 30 / 24), scaled to the image like the other lengths."""
    s = height / 480.0
    return dict(TC.scaled_thresholds(height), min_mask=max(int(20 * s), 1), min_bbox=max(int(30 * s), 1),
                min_side=max(int(24 * s), 1))


def run_tracker(render, device, H, W, n_objects, resolution, n_frames=3):
    """The online loop (track -> insert_scan) over the static scene of occserver_cases.make_frames (the same synthetic
    sequence, the same turned map frame) -> per frame (detection ids, remap incl. the counter, rendered label)."""
    from morefusion_amd import geometry, synthetic
    from morefusion_amd.contrib import InstanceTracker, OctomapServer
    server = OctomapServer(resolution=resolution, device=device)
    kw = dict(render="mesh", server=server) if render == "mesh" else {}
    trk = InstanceTracker(server.mapping, thresholds=thresholds(H), **kw)
    pitch_of = OC.make_pitch_of(W)
    out = []
    for f in synthetic.make_tracking_sequence(0, n_frames, H, W, n_objects=n_objects):
        K, T = f["K"], OC.G @ f["T_sensor_to_map"]
        pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2]).astype(np.float32)
        tracked, _, class_of, rendered = trk.track(pcd, f["label_detected"], f["class_ids_by_detection"], K, T,
                                                   depth=f["depth"] if render == "mesh" else None)
        server.insert_scan(trk.pts_map.reshape(H, W, 3), tracked, class_of, pitch_of, origin=T[:3, 3])
        out.append((list(trk.last["det_ids"]), trk.last["remap_host"].copy(), rendered))
    return out


def check_tracker_routes(device, H, W, n_objects, resolution):
    """From frame 1 on the mesh route assigns every detection the id the ray-cast route assigns it.  Checked on the
    emulator first: at 48 x 64 the ray-cast route itself loses objects (a map of one coarse frame is too sparse for its
    rays: new ids every frame), with 5 objects at 120 x 160 two of them overlap and one detection is vetoed in both
    routes; 3 objects at 96 x 128 and at 120 x 160 are matched by both routes in every frame."""
    ray = run_tracker("raycast", device, H, W, n_objects, resolution)
    mesh = run_tracker("mesh", device, H, W, n_objects, resolution)
    assert len(ray) == len(mesh) == 3
    for k, ((d_r, remap_r, rend_r), (d_m, remap_m, rend_m)) in enumerate(zip(ray, mesh)):
        assert d_r == d_m and len(d_r) == n_objects
        assert np.array_equal(remap_r, remap_m), (k, remap_r, remap_m)
        if k == 0:
            assert (rend_m == -2).all()  # no map yet: the service draws nothing
        else:
            assert (remap_r[:-1] >= 1).all() and remap_r[-1] == n_objects + 1  # every detection matched, no new id
            assert len(set(np.unique(rend_m).tolist()) - {-2}) == n_objects
