"""TEST HELPER: the scenes of tests/test_emul_occserver.py and tests/test_gpu_occserver.py.

Frames of ``synthetic.make_tracking_sequence`` (objects on a table in front of a wall).  The map frame is turned so that
the table top is the plane z = 0 with the objects above it (the server's ground plane), the tracked labels are made
from the ground truth (object i -> id i + 1), with a band of -2 around the image and one lone stride-2 background pixel
relabelled as instance ``LONE``: its single point only creates its cloud, so it never gets a centre."""
import numpy as np

import occserver_ref as S
import occtrack_cases as C
import occtrack_ref as T

LONE, LONE_CLASS = 9, 2
# map' = G map: x' = x, y' = z, z' = 0.2 - y (the table top y = 0.2, y pointing down, becomes z' = 0, z' pointing up)
G = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.2], [0, 0, 0, 1]], np.float64)


def make_frames(seed, H, W, n_objects, n_frames=3):
    from morefusion_amd import geometry, synthetic
    frames = []
    for f in synthetic.make_tracking_sequence(seed, n_frames, H, W, n_objects=n_objects):
        K = f["K"]
        pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        T_sensor_to_map = G @ f["T_sensor_to_map"]
        det = f["label_detected"]
        label = np.full((H, W), -1, np.int32)
        classes = {LONE: LONE_CLASS}
        for d, obj in f["object_of_detection"].items():
            label[det == d] = obj + 1
            classes[obj + 1] = int(f["class_ids"][obj])
        label[:2], label[-2:], label[:, :2], label[:, -2:] = -2, -2, -2, -2
        pts_map = T.transform(pcd, T_sensor_to_map).reshape(H, W, 3)
        jj, ii = np.nonzero((label[::2, ::2] == -1) & ~np.isnan(pts_map[::2, ::2]).any(axis=2))
        label[2 * jj[len(jj) // 3], 2 * ii[len(jj) // 3]] = LONE
        frames.append(dict(pts_map=pts_map, label=label, classes=classes, T_sensor_to_map=T_sensor_to_map,
                           origin=T_sensor_to_map[:3, 3].copy()))
    return frames


def insert(server, f, pitch_of, to=None):
    to = to or (lambda x: x)
    server.insert_scan(to(f["pts_map"]), to(f["label"]), f["classes"], pitch_of, origin=f["origin"])


def check_clean(server):
    assert int(server.mapping._overflow[0]) == 0
    for t in server.mapping._trees.values():
        assert t.bits is None or not bool(t.bits.any())


def run_sequence(frames, pitch_of, device, resolution):
    """Sequence A in lockstep with the mirror: after each frame the maps, centres and boxes are bitwise equal."""
    from morefusion_amd.contrib import OctomapServer
    server, ref = OctomapServer(resolution=resolution, device=device), S.OctomapServer(resolution=resolution)
    first = {}
    for f in frames:
        insert(server, f, pitch_of)
        insert(ref, f, pitch_of)
        S.maps_equal(server, ref)
        S.stats_equal(server, ref)
        check_clean(server)
        for i, c in ref.centers.items():
            assert first.setdefault(i, c.copy()).tobytes() == c.tobytes()  # a centre stays what its first frame made it
    ids = sorted(i for i in ref.octrees if i not in (S.BACKGROUND_ID, LONE))
    assert len(ids) >= 3 and set(ids) <= set(ref.centers) and S.BACKGROUND_ID in ref.centers
    assert any((ref.bbx[i][0] != ref.centers[i]).any() for i in ids)
    # the lone pixel: a map with its hits, but no centre, no box, not published
    assert LONE in server.mapping.instance_ids and len(S.known_cells(server.mapping, LONE)) >= 1
    assert LONE not in server.centers and LONE not in server.bbx and LONE not in ref.centers
    out = server.publish_grids(frames[-1]["T_sensor_to_map"])
    assert out["instance_ids"] == ids == ref.publish_grids(frames[-1]["T_sensor_to_map"])[0]["instance_ids"]
    return server, ref


def run_clamped(frame, pitch_of, device, resolution, times=5):
    """Sequence B: the same frame ``times`` times (the fifth hit reaches the clamp) -> (server, mirror)."""
    from morefusion_amd.contrib import OctomapServer
    server, ref = OctomapServer(resolution=resolution, device=device), S.OctomapServer(resolution=resolution)
    for _ in range(times):
        insert(server, frame, pitch_of)
        insert(ref, frame, pitch_of)
    S.maps_equal(server, ref)
    S.stats_equal(server, ref)
    assert any(v == ref.lo_max for v in ref.octrees[1].values.values())
    return server, ref


def check_publish(server, ref, T_sensor_to_map, ground, free):
    server.ground_as_noentry = ref.ground_as_noentry = ground
    server.free_as_noentry = ref.free_as_noentry = free
    got = server.publish_grids(T_sensor_to_map)
    exp, counts = ref.publish_grids(T_sensor_to_map)
    assert got["instance_ids"] == exp["instance_ids"] and got["class_ids"] == exp["class_ids"] and len(exp["instance_ids"]) >= 3
    for k, dtype in (("pitch", np.float32), ("origin", np.float64), ("grid_target", np.float32),
                     ("grid_noentry", np.float32), ("grid_nontarget_empty", np.bool_)):
        g = got[k].cpu().numpy()
        assert g.dtype == dtype and g.shape == exp[k].shape and np.array_equal(g, exp[k]), (k, ground, free)
    # a condition on the scene, asserted on the mirror alone: no branch is tested vacuously
    assert counts["own_occupied"] > 0 and counts["other_at_clamp"] > 0
    assert (counts["ground"] > 0) == ground and (counts["free_background"] > 0) == free
    if ground and free:
        assert counts["overwritten"] > 0
    return counts


make_pitch_of = C.make_pitch_of
