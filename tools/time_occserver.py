"""The map server's launches on one 480 x 640 frame of synthetic.make_tracking_sequence (8 instances): CUDA-event
medians of mf_occserver_bounds / _stats / _raycast / _apply on a server whose boxes already hold the frame, of
mf_occserver_publish for its B grids, the wall time of insert_scan and publish_grids with their read-backs, and, next
to them, MultiInstanceOctreeMapping.integrate_tracked_frame on the same frame (DESIGN.md "Map server").  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import _lib, geometry, synthetic  # noqa: E402
from morefusion_amd.contrib import MultiInstanceOctreeMapping, OctomapServer  # noqa: E402
from morefusion_amd.contrib.instance_tracking import transform_points  # noqa: E402
from morefusion_amd.contrib.multi_instance_octree_mapping import BACKGROUND_ID  # noqa: E402

TO_GROUND = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.2], [0, 0, 0, 1]], np.float64)


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    f = synthetic.make_tracking_sequence(0, 1)[0]
    H, W = f["label_detected"].shape
    K, T = f["K"], TO_GROUND @ f["T_sensor_to_map"]
    pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2]).astype(np.float32)
    pts_map = transform_points(torch.as_tensor(pcd).cuda(), T, "cuda").reshape(H, W, 3)
    label = np.full((H, W), -1, np.int32)
    classes = {}
    for d, obj in f["object_of_detection"].items():
        label[f["label_detected"] == d] = obj + 1
        classes[obj + 1] = int(f["class_ids"][obj])
    label_d = torch.as_tensor(label).cuda()
    pitch_of = lambda c: synthetic.CLASS_PITCH[int(c)]  # noqa: E731
    origin = T[:3, 3]
    server = OctomapServer()
    insert = lambda: server.insert_scan(pts_map, label_d, classes, pitch_of, origin=origin)  # noqa: E731
    insert()
    server.publish_grids(T)
    torch.cuda.synchronize()
    res = dict(H=H, W=W, n_instances=len(classes), reps=args.reps)
    res["insert_scan_wall_us"] = wall(insert, args.reps)
    res["publish_grids_wall_us"] = wall(lambda: server.publish_grids(T), args.reps)
    # the launches one by one, with insert_scan's arguments
    m, L, s = server.mapping, _lib.lib(), _lib.stream_ptr()
    ids = sorted(classes)
    pts, lab = m._points(pts_map), label_d.reshape(-1).contiguous()
    bg = m._index(BACKGROUND_ID)
    slots = m._slots([(i, m._index(i), 0) for i in ids] + [(-1, bg, 0)])
    n_slots, n_trees = len(ids) + 1, len(m._trees)
    bounds = torch.empty((n_trees, 6), dtype=torch.int32, device="cuda")
    table = torch.empty((n_slots + 1, 10), dtype=torch.float64, device="cuda")
    descs = m._descs().data_ptr()
    o = [float(np.float32(c)) for c in origin]
    cells = max(t.dim[0] * t.dim[1] * t.dim[2] for t in m._trees.values())
    res["bounds_us"] = events(lambda: L.mf_occserver_bounds(pts.data_ptr(), lab.data_ptr(), H, W, slots.data_ptr(), n_slots,
                                                            descs, bg, n_trees, bounds.data_ptr(), s), args.reps)
    res["stats_us"] = events(lambda: L.mf_occserver_stats(pts.data_ptr(), lab.data_ptr(), H, W, slots.data_ptr(), n_slots,
                                                          table.data_ptr(), s), args.reps)

    def cast_and_apply(cast, apply):
        def run():
            if cast:
                L.mf_occserver_raycast(pts.data_ptr(), lab.data_ptr(), H, W, slots.data_ptr(), n_slots, descs, bg, *o,
                                       m._overflow.data_ptr(), s)
            if apply:
                L.mf_occserver_apply(descs, n_trees, cells, float(server.lo_hit), float(server.lo_miss),
                                     float(server.lo_min), float(server.lo_max), s)
        return run
    both = events(cast_and_apply(True, True), args.reps)
    res["apply_us"] = events(cast_and_apply(False, True), args.reps)  # no bits set: every cell read, none written
    res["raycast_us"] = both - res["apply_us"]
    res["raycast_plus_apply_us"] = both
    grids = server.publish_grids(T)
    res["publish_B"] = len(grids["instance_ids"])
    order = torch.tensor([m._index(i) for i in sorted(m._trees)], dtype=torch.int32).cuda()
    target = torch.tensor([m._index(i) for i in grids["instance_ids"]], dtype=torch.int32).cuda()
    centers = torch.from_numpy(np.stack([server.centers[i] for i in grids["instance_ids"]])).cuda()
    inv = np.linalg.inv(T)
    Ts = torch.from_numpy(np.stack([inv, T]).astype(np.float32)).cuda()
    res["publish_us"] = events(lambda: L.mf_occserver_publish(
        descs, n_trees, order.data_ptr(), bg, target.data_ptr(), grids["pitch"].data_ptr(), centers.data_ptr(),
        Ts[0].data_ptr(), Ts[1].data_ptr(), server.prob_max, 3, len(target), 32, grids["origin"].data_ptr(),
        grids["grid_target"].data_ptr(), grids["grid_noentry"].data_ptr(), grids["grid_nontarget_empty"].data_ptr(), s),
        args.reps)
    res["box_cells"] = {str(k): int(np.prod(t.dim)) for k, t in m._trees.items()}
    res["overflow"] = int(m._overflow.cpu()[0])
    # the dataset model on the same frame: every instance carves its own map with its own rays
    mm = MultiInstanceOctreeMapping()
    tracked = lambda: mm.integrate_tracked_frame(pts_map, label_d, classes, pitch_of, origin=origin)  # noqa: E731
    tracked()
    res["integrate_tracked_frame_wall_us"] = wall(tracked, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
