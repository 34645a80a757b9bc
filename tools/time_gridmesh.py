"""The render-service route on one 480 x 640 frame of synthetic.make_tracking_sequence (8 instances) next to the
ray-cast route: CUDA-event medians of contrib.render_voxel_grids end to end (with its one read-back) and of
render_instance_maps on the same maps, and the split of the former -- grids_in_map_frame, count (with the read-back),
emit, adjacency, smooth, raster (setup + raster + resolve), label (DESIGN.md "Grid meshes").  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import geometry, synthetic  # noqa: E402
from morefusion_amd.contrib import OctomapServer, render_instance_maps, render_voxel_grids  # noqa: E402
from morefusion_amd.contrib.instance_tracking import transform_points  # noqa: E402
from morefusion_amd.geometry import grid_mesh  # noqa: E402
from morefusion_amd.geometry.render import RenderPlan  # noqa: E402

TO_GROUND = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.2], [0, 0, 0, 1]], np.float64)


def events(fn, reps, warmup=3):
    out = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    f = synthetic.make_tracking_sequence(0, 1)[0]
    H, W = f["label_detected"].shape
    K, T = f["K"], TO_GROUND @ f["T_sensor_to_map"]
    pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2]).astype(np.float32)
    pts_map = transform_points(torch.as_tensor(pcd).cuda(), T, "cuda")
    label = np.full((H, W), -1, np.int32)
    classes = {}
    for d, obj in f["object_of_detection"].items():
        label[f["label_detected"] == d] = obj + 1
        classes[obj + 1] = int(f["class_ids"][obj])
    server = OctomapServer()
    server.insert_scan(pts_map.reshape(H, W, 3), torch.as_tensor(label).cuda(), classes,
                       lambda c: synthetic.CLASS_PITCH[int(c)], origin=T[:3, 3])
    depth = torch.as_tensor(f["depth"]).cuda()
    grids = server.grids_in_map_frame()
    res = dict(height=H, width=W, instances=len(grids["instance_ids"]), reps=args.reps)
    res["render_voxel_grids_us"] = events(lambda: render_voxel_grids(server.grids_in_map_frame(), depth, K, T, H, W), args.reps)
    res["render_instance_maps_us"] = events(lambda: render_instance_maps(server.mapping, pts_map, K, T, H, W), args.reps)
    res["grids_in_map_frame_us"] = events(server.grids_in_map_frame, args.reps)
    plan = grid_mesh.GridMeshPlan(grids["grid"], grids["pitch"], grids["origin"])
    res["count_us"] = events(plan.count, args.reps)
    res["emit_us"] = events(plan.emit, args.reps)
    res["adjacency_us"] = events(plan.adjacency, args.reps)
    res["vertices"], res["faces"] = plan.n_vertices, plan.n_faces
    res["smooth_us"] = events(plan.smooth, args.reps)
    meshes = [m for m in plan.meshes() if m[1].shape[0]]
    rp = RenderPlan(meshes, np.stack([np.linalg.inv(T)] * len(meshes)), K, H, W, instance_ids=list(range(len(meshes))))
    res["raster_us"] = events(rp.run, args.reps)
    out = rp.run()
    res["label_us"] = events(lambda: grid_mesh.label_of_render(out["depth"][0], out["instance"][0], depth), args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
