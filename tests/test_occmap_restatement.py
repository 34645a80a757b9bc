"""Known answers of the occupancy-mapping restatement (tests/occmap_ref.py) that the HIP kernels are checked
against: OctoMap's insertPointCloud / updateNodes / leaf search and the reference's get_target_grids and
build_octomap, on hand-built scans whose rays stay off DDA ties."""
import numpy as np
import pytest

import occmap_ref as R

PITCH = 0.01


def _ray_keys(tree, o, end):
    return sorted(R.unpack(tree.compute_ray_keys(o, np.asarray([end], np.float32))).tolist())


def test_constants_are_octomaps_defaults():
    assert R.LO_HIT == np.float32(0.84729785) and R.LO_MISS == np.float32(-0.4054651)
    assert R.LO_MIN == np.float32(-2.000028) and R.LO_MAX == np.float32(3.5110307)
    assert abs(R.probability(R.LO_HIT) - 0.7) < 1e-7 and abs(R.probability(R.LO_MISS) - 0.4) < 1e-7


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_axis_aligned_ray_of_n_cells(n):
    t = R.OcTree(PITCH)
    o = np.float32([0.0025, 0.0051, 0.0052])
    end = np.float32([0.0025 + PITCH * n + 0.003, 0.0051, 0.0052])
    t.insert_point_cloud(end[None], o)
    k0 = R.KEY_MAX
    assert _ray_keys(t, o, end) == [[k0 + i, k0, k0] for i in range(n)]
    free = {int(R.pack([k0 + i, k0, k0])) for i in range(n)}
    occ = int(R.pack([k0 + n, k0, k0]))
    assert set(t.values) == free | {occ}
    assert all(t.values[c] == R.LO_MISS for c in free) and t.values[occ] == R.LO_HIT
    assert abs(R.probability(t.values[occ]) - 0.7) < 1e-7


def test_two_points_in_one_cell_give_one_hit():
    t = R.OcTree(PITCH)
    pts = np.float32([[0.0512, 0.0031, 0.1004], [0.0577, 0.0068, 0.1093]])  # one cell
    t.insert_point_cloud(pts, (0.0013, 0.0021, 0.0017))
    c = int(R.pack(t.keys(pts[:1])[0][0]))
    assert t.values[c] == R.LO_HIT


def test_free_for_one_point_and_occupied_for_another_gives_one_hit():
    t = R.OcTree(PITCH)
    o = np.float32([0.0025, 0.0051, 0.0052])
    near = np.float32([0.0325, 0.0051, 0.0052])    # ends in cell x + 3
    far = np.float32([0.0625, 0.0051, 0.0052])     # passes through cell x + 3
    t.insert_point_cloud(np.stack([near, far]), o)
    k0 = R.KEY_MAX
    assert t.values[int(R.pack([k0 + 3, k0, k0]))] == R.LO_HIT
    assert t.values[int(R.pack([k0 + 4, k0, k0]))] == R.LO_MISS


@pytest.mark.parametrize("k", [5, 6, 12])
def test_repeated_scans_clamp_exactly(k):
    t = R.OcTree(PITCH)
    o = np.float32([0.0025, 0.0051, 0.0052])
    end = np.float32([0.0525, 0.0051, 0.0052])
    for _ in range(k):
        t.insert_point_cloud(end[None], o)
    k0 = R.KEY_MAX
    occ, free = t.values[int(R.pack([k0 + 5, k0, k0]))], t.values[int(R.pack([k0 + 2, k0, k0]))]
    assert occ == R.LO_MAX  # 5 hits: 4.24 > 3.511
    expect_free = np.float32(0)
    for _ in range(k):
        expect_free = R.clamp_add(expect_free, R.LO_MISS)
    assert free == expect_free and (k < 5 or free == R.LO_MIN)


def test_update_applies_one_hit_per_point_without_merging():
    t = R.OcTree(PITCH)
    p = np.float32([[0.0512, 0.0031, 0.1004]])
    t.update_nodes(np.concatenate([p, p, p]))
    c = int(R.pack(t.keys(p)[0][0]))
    assert t.values[c] == R.clamp_add(R.clamp_add(R.LO_HIT, R.LO_HIT), R.LO_HIT)


def _scan_along_x(mapping, iid, n_scans=1, y=0.0051, x_end=0.0525):
    pcd = np.float32([[[x_end, y, 0.0052]]])
    for _ in range(n_scans):
        mapping.integrate(iid, np.ones((1, 1), bool), pcd, origin=(0.0025, y, 0.0052))


def test_unknown_cells_appear_in_no_grid():
    m = R.MultiInstanceOctreeMapping()
    m.initialize(1, pitch=PITCH)
    _scan_along_x(m, 1)
    for g in m.get_target_grids(1, dimensions=(8, 8, 8), pitch=PITCH, origin=(1.0, 1.0, 1.0)):
        assert not g.any()
    gt, gn, ge = m.get_target_grids(1, dimensions=(8, 2, 2), pitch=PITCH, origin=(0.005, 0.005, 0.005))
    assert gt[5, 0, 0] == np.float32(R.probability(R.LO_HIT)) and (gt > 0).sum() == 1
    assert (ge[:5, 0, 0] == np.float32(1 - R.probability(R.LO_MISS))).all() and (ge > 0).sum() == 5
    assert not gn.any()


@pytest.mark.parametrize("order", [(1, 2), (2, 1)])
def test_two_instances_over_one_voxel_last_writer_wins(order):
    m = R.MultiInstanceOctreeMapping()
    scans = {1: 1, 2: 3}  # instance 2 is hit three times: a different occupancy
    for iid in order:
        m.initialize(iid, pitch=PITCH)
        _scan_along_x(m, iid, scans[iid])
    m.initialize(9, pitch=PITCH)
    _, gn, ge = m.get_target_grids(9, dimensions=(8, 2, 2), pitch=PITCH, origin=(0.005, 0.005, 0.005))
    last = m.octrees[order[-1]]
    k0 = R.KEY_MAX
    assert gn[5, 0, 0] == np.float32(R.probability(last.values[int(R.pack([k0 + 5, k0, k0]))]))
    assert ge[2, 0, 0] == np.float32(1 - R.probability(last.values[int(R.pack([k0 + 2, k0, k0]))]))
    gt, gn2, _ = m.get_target_grids(order[0], dimensions=(8, 2, 2), pitch=PITCH, origin=(0.005, 0.005, 0.005))
    assert gt[5, 0, 0] > 0.5 and gn2[5, 0, 0] == gn[5, 0, 0]


def _tiny_frame():
    pcd = np.full((2, 3, 3), np.nan)
    pcd[0, 0] = [0.0525, 0.0051, 0.0052]
    pcd[0, 1] = [0.0525, 0.0051, 0.0052]
    pcd[0, 2] = [0.0825, 0.0051, 0.0052]
    pcd[1, 0] = [0.0525, 0.0151, 0.0052]
    pcd[1, 1] = [0.0825, 0.0151, 0.0052]
    label = np.array([[3, 5, 3], [4, 7, 0]], np.int32)
    return pcd, label


def test_class_id_zero_instances_are_mapped_nowhere():
    pcd, label = _tiny_frame()
    m = R.build_octomap(pcd, label, [4, 7], [0, 2], lambda c: PITCH)
    assert list(m.octrees) == [7, 0]
    fg_key = int(R.pack(m.octrees[0].keys(pcd[1, 0][None])[0][0]))
    assert fg_key not in m.octrees[0].values  # instance 4's point: neither in 4 (class 0) nor in the background


def test_background_labels_are_separate_ordered_scans():
    pcd, label = _tiny_frame()
    m = R.build_octomap(pcd, label, [4, 7], [0, 2], lambda c: PITCH)
    bg = m.octrees[0].values
    k0 = R.KEY_MAX
    # labels 3 and 5 both end in cell x + 5: one hit per scan, two scans -> two hits
    assert bg[int(R.pack([k0 + 5, k0, k0]))] == R.clamp_add(R.LO_HIT, R.LO_HIT)
    # cell x + 2 is free in the scans of labels 3 (twice in one scan) and 5: two misses, in np.unique order
    assert bg[int(R.pack([k0 + 2, k0, k0]))] == R.clamp_add(R.LO_MISS, R.LO_MISS)
    merged = R.OcTree(PITCH)
    pts = pcd.reshape(-1, 3)[np.isin(label.reshape(-1), [0, 3, 5])]
    merged.insert_point_cloud(pts, (0, 0, 0))
    assert merged.values != bg  # one merged scan is NOT what the reference computes
