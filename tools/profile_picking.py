#!/usr/bin/env python
"""Event timings of contrib.occlusion_analysis (csrc/render.hip + csrc/pickorder.hip): medians of 20 launches after
warm-up, 8 YCB objects at 480 x 640 (16 render items into 9 targets).  Prints CSV rows case,stage,median_us,min_us
for profiles/picking_kernel_table.csv; ``analysis`` is the whole call with its host part (buffers, the copy back,
the ratio and the quaternions), timed with a host clock around a device synchronise."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import morefusion_amd as mf  # noqa: E402
from morefusion_amd.contrib.picking_order import OcclusionPlan  # noqa: E402
from tools.profile_render import meshes, time_stage  # noqa: E402


def main():
    H, W = 480, 640
    K = np.array([[619.4, 0, 319.7], [0, 618.9, 240.7], [0, 0, 1]])
    ycb = meshes()
    rs = np.random.RandomState(0)
    n = 8
    Ts = np.stack([np.eye(4)] * n)
    for i in range(n):  # two rows of four, the near row over the far one
        Ts[i, :3, :3] = mf.synthetic.random_rotation(rs)
        Ts[i, :3, 3] = (-0.21 + 0.14 * (i % 4) + rs.uniform(-0.02, 0.02), 0.02 * (i // 4), 0.55 + 0.2 * (i // 4))
    index = [i % 3 for i in range(n)]
    plan = OcclusionPlan(ycb, Ts, K, H, W, mesh_index=index)
    out = {k: v.cpu().numpy() for k, v in plan.run().items()}
    torch.cuda.synchronize()
    print("case,stage,median_us,min_us")
    r = plan.plan
    rows = [("render_setup", r.setup, None), ("render_raster", r.raster, r.setup), ("render_resolve", r.resolve, None),
            ("pick_occlusion", plan.occlusion, None), ("pick_grasp", plan.grasp, None), ("all_launches", plan.run, None)]
    for stage, fn, before in rows:
        med, lo = time_stage(fn, before)
        print(f"analysis8,{stage},{med:.1f},{lo:.1f}")
    pcd = torch.as_tensor(mf.geometry.pointcloud_from_depth(r.out["depth"][0].cpu().numpy(), K[0, 0], K[1, 1], K[0, 2],
                                                            K[1, 2])).cuda()
    med, lo = time_stage(lambda: mf.geometry.estimate_pointcloud_normals(pcd))
    print(f"analysis8,pick_normals_full_image,{med:.1f},{lo:.1f}")
    ts = []
    for k in range(25):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mf.contrib.occlusion_analysis(ycb, Ts, K, H, W, mesh_index=index)
        torch.cuda.synchronize()
        if k >= 5:
            ts.append((time.perf_counter() - t0) * 1e6)
    print(f"analysis8,analysis_with_host,{np.median(ts):.1f},{np.min(ts):.1f}")
    off = out["occluded_by"][~np.eye(n, dtype=bool)]
    print(f"# analysis8: {r.total} face records, {r.n_targets} x {H} x {W} px, whole {out['whole'].tolist()}, "
          f"{int((off > 0).sum())} occluding pairs, {int(off.sum())} hidden px", flush=True)


if __name__ == "__main__":
    main()
