#!/usr/bin/env python
"""OccupancyRegistration for every object of a frame in one call -- counterpart of the inner loop of the reference's
examples/ycb_video/dense_fusion/eval_densefusion_occupancy.py:76-131.

A frame of boxes at known poses (``synthetic.make_cad_frame``) -> ``MultiInstanceOctreeMapping.integrate_frame`` ->
per object ``get_target_grids`` at 16^3 with pitch = bounding-box diagonal / 16 around the initial pose -> the CAD
cloud voxel-down-sampled at that pitch -> ONE ``contrib.occupancy_registration_batch`` call (threshold 2, alpha
0.01, 100 iterations) -> ADD / ADD-S before and after through ``metrics.average_distance_device``.  The initial
poses are the truth perturbed by a few degrees and millimetres (the reference starts from DenseFusion's poses).
At this coarse pitch (about 10 mm) and from one view the loss falls but ADD need not: DESIGN.md "Occupancy
registration" has the measured figures.

    python examples/pose_refinement_occupancy.py [--objects 3] [--iterations 100]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as morefusion  # noqa: E402


def box_mesh(half):
    hx, hy, hz = half
    v = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, faces


def box_cloud(half, step=0.004):
    """Points on the six faces of the box, ``step`` apart."""
    axes = [np.arange(-h, h + 1e-9, step) for h in half]
    pts = []
    for a in range(3):
        u, v = [axes[k] for k in range(3) if k != a]
        uu, vv = np.meshgrid(u, v, indexing="ij")
        for s in (-half[a], half[a]):
            p = np.zeros(uu.shape + (3,))
            p[..., a] = s
            p[..., [k for k in range(3) if k != a][0]] = uu
            p[..., [k for k in range(3) if k != a][1]] = vv
            pts.append(p.reshape(-1, 3))
    return np.unique(np.round(np.concatenate(pts), 6), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    halves = {2: (0.05, 0.035, 0.06), 5: (0.04, 0.04, 0.07), 9: (0.06, 0.03, 0.045)}
    meshes = {c: box_mesh(h) for c, h in halves.items()}
    frame = morefusion.synthetic.make_cad_frame(meshes, seed=args.seed, n_objects=args.objects)
    K = frame["K"]
    to_gpu = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    pcd = morefusion.geometry.pointcloud_from_depth(frame["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    mapping = morefusion.contrib.MultiInstanceOctreeMapping()
    mapping.integrate_frame(to_gpu(pcd.astype(np.float32)), frame["label"], frame["instance_ids"], frame["class_ids"],
                            lambda c: 0.005)

    rs = np.random.RandomState(args.seed + 1)
    dim = 16
    clouds, sources, grids, pitches, origins, inits = [], [], [], [], [], []
    for ins, cls, T_true in zip(frame["instance_ids"].tolist(), frame["class_ids"].tolist(), frame["Ts_cad2cam"]):
        cad = box_cloud(halves[cls])
        dT = np.eye(4)
        dT[:3, :3] = morefusion.synthetic.random_rotation(rs, np.deg2rad(5))
        dT[:3, 3] = rs.uniform(-0.004, 0.004, 3)
        C = np.eye(4)
        C[:3, 3] = T_true[:3, 3]
        T_init = C @ dT @ np.linalg.inv(C) @ T_true
        pitch = float(np.linalg.norm(cad.max(0) - cad.min(0))) / dim  # eval_densefusion_occupancy.py:85-87
        centre = T_init[:3, 3] + T_init[:3, :3] @ ((cad.max(0) + cad.min(0)) / 2)
        origin = centre - pitch * (dim / 2.0 - 0.5)
        target, nontarget, empty = mapping.get_target_grids(ins, dimensions=(dim,) * 3, pitch=pitch, origin=origin)
        grids.append(np.stack([target, nontarget, empty]).astype(np.float32))
        sources.append(morefusion.extra.open3d.voxel_down_sample(cad, pitch).astype(np.float32))
        clouds.append(cad)
        pitches.append(pitch)
        origins.append(origin.astype(np.float32))
        inits.append(T_init.astype(np.float32))

    inits = np.stack(inits)
    transform, nan, losses, _ = morefusion.contrib.occupancy_registration_batch(
        sources, grids, pitch=pitches, origin=np.stack(origins), threshold=2, transforms_init=inits,
        iteration=args.iterations, alpha=0.01, return_history=True)
    B = len(clouds)
    true = np.concatenate([frame["Ts_cad2cam"]] * 2)
    pred = torch.cat([to_gpu(inits), transform])
    add, add_s = morefusion.metrics.average_distance_device(clouds, true, pred, cloud_index=list(range(B)) * 2)
    add, add_s, losses, nan = add.cpu().numpy(), add_s.cpu().numpy(), losses.cpu().numpy(), nan.cpu().numpy()
    for b in range(B):
        print(f"instance {frame['instance_ids'][b]} (class {frame['class_ids'][b]}, {len(sources[b])} points, pitch "
              f"{pitches[b] * 1000:.1f} mm): loss {losses[0, b]:.4f} -> {losses[-1, b]:.4f}, "
              f"ADD {add[b] * 1000:.2f} -> {add[B + b] * 1000:.2f} mm, ADD-S {add_s[b] * 1000:.2f} -> "
              f"{add_s[B + b] * 1000:.2f} mm{' (NaN: kept the initial pose)' if nan[b] else ''}")


if __name__ == "__main__":
    main()
