#!/usr/bin/env python
"""Regenerate tests/golden/ref_pointcloud_normals.npz: float64 organised point images and the normals that the
reference's own ``_estimate_pointcloud_normals_organized`` returns for them.

    python tools/gen_pointcloud_normals_golden.py <reference checkout> [output.npz]

The reference module (morefusion/geometry/estimate_pointcloud_normals.py) is loaded from the checkout at run time,
with an empty stand-in for ``open3d`` (only the unorganised path uses it); nothing of it is copied here.  Not run by
any test: the committed file is the record.
"""
import importlib.util
import os
import sys
import types

import numpy as np

H, W = 24, 32


def inputs():
    """-> {name: float64 [H, W, 3]}: a tilted plane, a sphere cap, the plane with a NaN block and a depth step."""
    i, j = np.mgrid[:H, :W].astype(np.float64)
    rx, ry = (j - 15.3) / 40.0, (i - 11.6) / 40.0  # the rays of a small pinhole camera
    z = 0.7 / (1.0 - 0.35 * rx + 0.2 * ry)  # the plane z = 0.35 x - 0.2 y + 0.7 along them
    plane = np.stack([rx * z, ry * z, z], -1)
    x, y = (j - 15.5) * 0.004, (i - 11.5) * 0.004  # a cap of the sphere of radius 0.09 around (0, 0, 0.6)
    cap = np.stack([x, y, 0.6 - np.sqrt(0.09 ** 2 - x * x - y * y)], -1)
    broken = plane.copy()
    broken[5:11, 7:15] = np.nan
    broken[:, 22:, 2] += 0.15  # a depth step between columns 21 and 22
    broken[17, 3] = np.nan
    return dict(plane=plane, sphere_cap=cap, plane_nan_step=broken)


def main():
    ref_root = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_pointcloud_normals.npz")
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    path = os.path.join(ref_root, "morefusion", "geometry", "estimate_pointcloud_normals.py")
    spec = importlib.util.spec_from_file_location("_ref_estimate_pointcloud_normals", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    data = {}
    for name, points in inputs().items():
        with np.errstate(all="ignore"):
            normals = mod._estimate_pointcloud_normals_organized(points.copy())
        assert normals.shape == points.shape and normals.dtype == np.float64
        data[f"points_{name}"], data[f"normals_{name}"] = points, normals
        print(f"{name}: {int(np.isnan(normals).any(axis=2).sum())} of {H * W} pixels without a normal")
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
