"""Time mf_tsdf_raycast against mf_tsdf_block_summary + mf_tsdf_render on the workload of tools/time_tsdf.py: frame 0 of
make_tracking_sequence(0, 2) at 480 x 640 fused into a 256^3 volume (6.25 mm voxels, truncation 4 voxels, ray step 2
voxels), rendered from frame 1's pose.  Device events around 20 calls, the smallest and the largest of 5 windows after
warm-up, the two kernels alternating in one process; one JSON line (DESIGN.md "TSDF render").  For B = 4, 8, 16: the
summary alone, the render alone on a summary made before (not the product's default: TsdfVolume.render makes the summary
on every call), the two together as TsdfVolume.render runs them, the block codes, and from stats_out the sums of
``sampled`` and ``visited`` next to the rays' samples (counted by a render whose summary says MIXED everywhere).  Every
render's depth and code are compared with the ray-cast's before anything is timed.

    python tools/time_tsdf_render.py [--out timing.json]
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
H, W = 480, 640


def timed(fn, reps=20):
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
ref_depth, ref_code = vol.raycast(K, T1, H, W, return_code=True)
out = {"raycast_codes": torch.bincount(ref_code.flatten().long(), minlength=5).cpu().tolist()}
# every sample "MIXED": visited = the rays' samples
_, stats = vol.render(K, T1, H, W, block=8, summary=torch.zeros(vol.summary_shape(8), dtype=torch.uint8, device="cuda"),
                      return_stats=True)
out["samples"] = int(stats[..., 1].sum())
out["raycast_ms"] = timed(lambda: vol.raycast(K, T1, H, W))
for B in (4, 8, 16):
    summary = vol.block_summary(B)
    got_depth, got_code, stats = vol.render(K, T1, H, W, block=B, summary=summary, return_code=True, return_stats=True)
    assert torch.equal(got_depth, ref_depth) and torch.equal(got_code, ref_code), B
    out[f"B{B}"] = {
        "blocks_mixed_free_unknown": torch.bincount(summary.flatten().long(), minlength=3).cpu().tolist(),
        "sampled": int(stats[..., 0].sum()), "visited": int(stats[..., 1].sum()),
        "summary_ms": timed(lambda: vol.block_summary(B)),
        "render_given_summary_ms": timed(lambda: vol.render(K, T1, H, W, block=B, summary=summary)),
        "summary_and_render_ms": timed(lambda: vol.render(K, T1, H, W, block=B)),
    }
out["raycast_again_ms"] = timed(lambda: vol.raycast(K, T1, H, W))
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh)
