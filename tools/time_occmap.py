"""One 480 x 640 occupancy frame (synthetic.make_occupancy_frame: 8 objects + wall / table background):
integrate_frame + get_target_grids_batch(network_inputs=True) on the device, REPS times after a warm-up,
wall time per frame with the host readback included (CUDA events); ``--ref`` adds the restatement's
CPU time (tests/occmap_ref.py) for the same frame.  Run under ``rocprofv3 --kernel-trace --stats`` for
the kernel table (DESIGN.md "Occupancy mapping")."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import geometry, synthetic  # noqa: E402
from morefusion_amd.contrib import MultiInstanceOctreeMapping  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    f = synthetic.make_occupancy_frame(0)
    K = f["K"]
    pcd = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pitch_of = lambda c: synthetic.CLASS_PITCH[int(c)]  # noqa: E731
    pitch = np.array([pitch_of(c) for c in f["class_ids"]])
    origin = np.stack([np.nanmedian(pcd[f["label"] == i], axis=0) for i in f["instance_ids"]]) - 15.5 * pitch[:, None]
    pcd_d = torch.as_tensor(pcd.astype(np.float32)).cuda()
    pitch_d, origin_d = torch.as_tensor(pitch).cuda(), torch.as_tensor(origin).cuda()

    def frame():
        m = MultiInstanceOctreeMapping()
        m.integrate_frame(pcd_d, f["label"], f["instance_ids"], f["class_ids"], pitch_of)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        out = m.get_target_grids_batch(f["instance_ids"], pitch_d, origin_d, network_inputs=True)
        return m, e, out

    frame()
    torch.cuda.synchronize()
    times, extract = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        m, e, _ = frame()
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        extract.append(e.elapsed_time(e1) * 1e-3)
    cells = {str(k): int(np.prod(t.dim)) for k, t in m._trees.items()}
    res = dict(frame_wall_ms=1e3 * float(np.median(times)), extract_ms=1e3 * float(np.median(extract)),
               box_cells=cells, valid_points=int((~np.isnan(pcd).any(axis=2)).sum()))
    if args.ref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import occmap_ref as R
        t0 = time.perf_counter()
        r = R.build_octomap(pcd, f["label"], f["instance_ids"], f["class_ids"], pitch_of)
        t1 = time.perf_counter()
        for tid, p, o in zip(f["instance_ids"], pitch, origin):
            r.get_target_grids(tid, dimensions=(32, 32, 32), pitch=p, origin=o)
        res.update(ref_integrate_s=t1 - t0, ref_grids_s=time.perf_counter() - t1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
