#!/usr/bin/env python
"""Time csrc/meshsdf.hip: the 64^3 solid-grid launch and the get_sdf query launch, for one class and for every
class of a model directory (YCBVideoModels layout) in one launch per stage.

    python tools/time_mesh_sdf.py MODEL_DIR [--class-id 2] [--reps 5]

Prints per launch the median device time (torch.cuda events, after one warm-up) and the point-triangle
evaluations per second (queries x faces / time)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402
from morefusion_amd.geometry import mesh_sdf  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def run(label, ycb, ids, reps):
    cads = [ycb.get_cad(c) for c in ids]
    meshes = [(torch.from_numpy(c.vertices).cuda(), torch.from_numpy(c.faces).cuda()) for c in cads]
    F = [len(c.faces) for c in cads]
    D = 64
    M = mesh_sdf._Meshes(meshes, torch.device("cuda"))
    t_prep = timed(lambda: mesh_sdf._Meshes(meshes, torch.device("cuda")), reps)
    params = [mesh_sdf.grid_params(v, D) for v, _ in meshes]
    origin = torch.stack([p[0] for p in params]).contiguous()
    h = torch.stack([p[1] for p in params]).contiguous()
    t_grid = timed(lambda: M.query([D ** 3] * len(ids), grid_origin=origin, grid_h=h, grid_dim=D,
                                   outputs=("occupancy",)), reps)
    grids = mesh_sdf.solid_voxel_grid_batch(meshes, D)
    pts = [morefusion.extra.open3d.voxel_down_sample(g.points, ycb.get_voxel_pitch(32, c)) for g, c in zip(grids, ids)]
    packed = torch.cat(pts)
    t_query = timed(lambda: M.query([len(p) for p in pts], points=packed, outputs=("sdf", "dist", "face", "winding")),
                    reps)
    ev_grid = sum(D ** 3 * f for f in F)
    ev_query = sum(len(p) * f for p, f in zip(pts, F))
    print(f"{label}: {len(ids)} meshes, {sum(F)} faces")
    print(f"  prepare (incl. packing)  {t_prep * 1e3:9.3f} ms")
    print(f"  solid grid {D}^3        {t_grid * 1e3:9.3f} ms  {ev_grid:.3e} evaluations  {ev_grid / t_grid:.3e} /s")
    print(f"  get_sdf query ({sum(len(p) for p in pts)} pts) {t_query * 1e3:9.3f} ms  {ev_query:.3e} evaluations  "
          f"{ev_query / t_query:.3e} /s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_dir")
    ap.add_argument("--class-id", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ycb = morefusion.datasets.YCBVideoModels(args.model_dir)
    run(f"class {args.class_id} ({ycb.class_names[args.class_id]})", ycb, [args.class_id], args.reps)
    run("all classes", ycb, list(range(1, len(ycb.class_names))), args.reps)


if __name__ == "__main__":
    main()
