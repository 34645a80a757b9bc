#!/usr/bin/env python
"""OBJ meshes -> the npz mesh fixtures of tests/golden (``vertices`` float64 as parsed, ``faces`` int32).

    python tools/make_mesh_fixtures.py SRC_DIR OUT_DIR [--classes 003_cracker_box 004_sugar_box ...]

SRC_DIR holds one ``<NNN_name>/`` directory per class with ``textured_simple.obj`` or ``textured.obj`` (the
YCBVideoModels layout); each becomes ``OUT_DIR/ycb_mesh_<NNN_name>.npz``.  Only the geometry is kept."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morefusion_amd.geometry.mesh_sdf import load_obj  # noqa: E402

DEFAULT_CLASSES = ("003_cracker_box", "004_sugar_box", "010_potted_meat_can")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--classes", nargs="*", default=list(DEFAULT_CLASSES), help="class directories (default: the "
                    "three fixture classes); 'all' = every class directory")
    args = ap.parse_args()
    classes = sorted(os.listdir(args.src_dir)) if args.classes == ["all"] else args.classes
    os.makedirs(args.out_dir, exist_ok=True)
    for name in classes:
        d = os.path.join(args.src_dir, name)
        obj = next((os.path.join(d, f) for f in ("textured_simple.obj", "textured.obj")
                    if os.path.exists(os.path.join(d, f))), None)
        if obj is None:
            print(f"skip {name}: no OBJ")
            continue
        v, f = load_obj(obj)
        out = os.path.join(args.out_dir, f"ycb_mesh_{name}.npz")
        np.savez_compressed(out, vertices=v, faces=f)
        print(f"{out}: {len(v)} vertices, {len(f)} faces, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
