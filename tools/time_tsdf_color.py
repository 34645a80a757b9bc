"""Time the TSDF colour on the workload of tools/time_tsdf.py: frames of make_tracking_sequence(0, 2) at 480 x 640 fused
into a 256^3 volume (6.25 mm voxels, truncation 4 voxels).  Device events around every call, the median (and the smallest
and largest) of 30 calls after warm-up, the variants alternating in one process; one JSON line (DESIGN.md "TSDF colour"):
``integrate`` alone, ``integrate`` with ``color``, the colour launch alone (mf_tsdf_integrate_colors through the volume's
own wrapper), ``color_image`` on the ray-cast from frame 1's pose, ``extract_mesh`` and ``sample_colors`` on its vertices.

    python tools/time_tsdf_color.py [--out timing.json]
"""
import argparse
import json
import os
import statistics
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
rgb = torch.as_tensor(frames[0]["rgb"]).cuda()
T0, T1 = (torch.as_tensor(f["T_sensor_to_map"]).cuda() for f in frames)
H, W = depth.shape
assert (H, W) == (480, 640) and rgb.dtype == torch.uint8
plain = TsdfVolume((256, 256, 256), 1.6 / 256, (-0.8, -0.9, 0.2))
vol = TsdfVolume((256, 256, 256), 1.6 / 256, (-0.8, -0.9, 0.2), colors=True)


def timed(fn, calls=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


vol.integrate(depth, K, T0, color=rgb)
plain.integrate(depth, K, T0)
assert torch.equal(vol.volume, plain.volume)
camera = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
d3 = depth[None].contiguous()
out = {"coloured_voxels": int((vol.colors[..., 3] > 0).sum()), "updated_voxels": int((vol.weight > 0).sum())}
out["integrate"] = timed(lambda: plain.integrate(depth, K, T0))
out["integrate_with_color"] = timed(lambda: vol.integrate(depth, K, T0, color=rgb))
out["color_launch_alone"] = timed(lambda: vol._integrate_colors(d3, rgb, camera, T0, None))
out["integrate_again"] = timed(lambda: plain.integrate(depth, K, T0))
render = vol.raycast(K, T1, H, W)
out["pixels_with_depth"] = int((render > 0).sum())
out["color_image"] = timed(lambda: vol.color_image(render, K, T1))
out["pixels_coloured"] = int((vol.color_image(render, K, T1)[..., 3] == 255).sum())
vertices, faces = vol.extract_mesh()
out["vertices"] = len(vertices)
out["extract_mesh"] = timed(lambda: vol.extract_mesh(), calls=10)
out["sample_colors"] = timed(lambda: vol.sample_colors(vertices))
out["vertices_coloured"] = int((vol.sample_colors(vertices)[:, 3] == 255).sum())
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh)
