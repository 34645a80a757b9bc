"""Time mf_tsdfmesh_count, mf_tsdfmesh_emit and the whole TsdfVolume.extract_mesh call (with its read-back of the two
totals and its allocations) with device events: 20 calls per window, the smallest and the largest of 5 windows after
warm-up, one JSON line (DESIGN.md "TSDF mesh").  The set-up is that of tools/time_tsdf.py: frame 0 of
make_tracking_sequence(0, 2) at 480 x 640 into 256^3 voxels of 6.25 mm.  The count reads the 134 MB volume once; its
bytes per second are those over the time (the volume fits the Infinity Cache and the loop re-reads it: not an HBM
figure).

    python tools/time_tsdfmesh.py [--out timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morefusion_amd import _lib, synthetic  # noqa: E402
from morefusion_amd.contrib import TsdfVolume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the JSON line to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the MI355X"
frames = synthetic.make_tracking_sequence(0, 2)
depth = torch.as_tensor(frames[0]["depth"]).cuda()
T0 = torch.as_tensor(frames[0]["T_sensor_to_map"]).cuda()
vol = TsdfVolume((256, 256, 256), 1.6 / 256, (-0.8, -0.9, 0.2))
vol.integrate(depth, frames[0]["K"], T0)


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


L = _lib.lib()
MIN_WEIGHT = 1.0
ws = torch.empty(L.mf_tsdfmesh_workspace_bytes(*vol.dims) // 8 + 2, dtype=torch.float64, device="cuda")
totals = torch.empty(2, dtype=torch.int64, device="cuda")


def count():
    _lib.check(L.mf_tsdfmesh_count(vol.volume.data_ptr(), *vol.dims, MIN_WEIGHT, ws.data_ptr(), totals.data_ptr(),
                                   _lib.stream_ptr()), "mf_tsdfmesh_count")


count()
V, F = totals.cpu().tolist()
vertices = torch.empty((V, 3), dtype=torch.float64, device="cuda")
faces = torch.empty((F, 3), dtype=torch.int32, device="cuda")
normals = torch.empty((V, 3), dtype=torch.float64, device="cuda")


def emit(with_normals):
    _lib.check(L.mf_tsdfmesh_emit(vol.volume.data_ptr(), *vol.dims, *vol.origin, vol.pitch, MIN_WEIGHT, ws.data_ptr(),
                                  V, F, vertices.data_ptr(), faces.data_ptr(),
                                  normals.data_ptr() if with_normals else None, _lib.stream_ptr()), "mf_tsdfmesh_emit")


volume_bytes = vol.volume.numel() * 4
out = {"voxels": vol.volume.numel() // 2, "vertices": V, "faces": F, "workspace_bytes": ws.numel() * 8 - 16,
       "volume_bytes": volume_bytes}
out["count_ms"] = timed(count, 20)
out["count_volume_GBps"] = [volume_bytes / (ms * 1e-3) / 1e9 for ms in reversed(out["count_ms"])]
out["emit_ms"] = timed(lambda: emit(False), 20)
out["emit_with_normals_ms"] = timed(lambda: emit(True), 20)
out["extract_mesh_ms"] = timed(lambda: vol.extract_mesh(), 20)
out["extract_mesh_with_normals_ms"] = timed(lambda: vol.extract_mesh(normals=True), 20)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh)
