"""Time mf_tsdf_integrate and mf_tsdf_raycast at 480 x 640 into a 256^3 volume (6.25 mm voxels, truncation 4 voxels,
ray step 2 voxels) with device events: 20 calls per window, the smallest and the largest of 5 windows after warm-up,
one JSON line (DESIGN.md "TSDF fusion").  The integrate's traffic is 8 bytes read per voxel and 8 bytes written per
touched voxel (counted from the weights after one integrate of a fresh volume); its bandwidth is that over the time.

    python tools/time_tsdf.py [--out timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import synthetic  # noqa: E402
from morefusion_amd.contrib import TsdfVolume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the JSON line to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
frames = synthetic.make_tracking_sequence(0, 2)
K = frames[0]["K"]
depth = torch.as_tensor(frames[0]["depth"]).cuda()
T0, T1 = (torch.as_tensor(f["T_sensor_to_map"]).cuda() for f in frames)
vol = TsdfVolume((256, 256, 256), 1.6 / 256, (-0.8, -0.9, 0.2))


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return min(ts), max(ts)


vol.integrate(depth, K, T0)
touched = int((vol.weight > 0).sum())
n_voxels = vol.volume.numel() // 2
out = {"voxels": n_voxels, "touched": touched}
out["integrate_ms"] = timed(lambda: vol.integrate(depth, K, T0), 20)
traffic = 8 * n_voxels + 8 * touched
out["integrate_GBps"] = [traffic / (ms * 1e-3) / 1e9 for ms in reversed(out["integrate_ms"])]
skip = torch.ones(1, dtype=torch.int32, device="cuda")
out["integrate_skipped_ms"] = timed(lambda: vol.integrate(depth, K, T0, skip_if=skip), 20)
out["raycast_ms"] = timed(lambda: vol.raycast(K, T1, 480, 640), 20)
ray_depth, code = vol.raycast(K, T1, 480, 640, return_code=True)
out["raycast_max_steps"] = vol.max_steps(vol.truncation / 2.0)
out["raycast_codes"] = torch.bincount(code.flatten().long(), minlength=5).cpu().tolist()
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh)
