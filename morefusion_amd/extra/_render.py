"""render_cad -- morefusion/extra/_pybullet.py:250-288 on the package's own rasteriser (csrc/render.hip).

The reference opens a pybullet OpenGL context, loads the CAD file and renders it once per transform with the
frustum ``computeProjectionMatrixFOV(fovy, width / height)``: square pixels, the principal point at the image
centre whatever the frame's intrinsics say.  The same frustum as a pinhole: fy = (height / 2) / tan(fovy / 2),
fx = fy, cx = width / 2 - 0.5, cy = height / 2 - 0.5 (pixel centres at half-integers of the GL viewport).  All
transforms are one launch, one target image each.  Colour is not rendered (``get_example`` discards it); pixel
parity with OpenGL is unpinned (DESIGN.md "Mesh rendering").
"""
import math
import os

import numpy as np

from ..geometry import mesh_sdf
from ..geometry import render as render_module


def fovy_intrinsics(fovy, height, width):
    """The 3 x 3 pinhole matrix of the reference's frustum; ``fovy`` in degrees (pybullet, trimesh's camera.fov)."""
    fy = (height / 2.0) / math.tan(math.radians(fovy) / 2.0)
    return np.array([[fy, 0.0, width / 2.0 - 0.5], [0.0, fy, height / 2.0 - 0.5], [0.0, 0.0, 1.0]])


def render_cad(cad, Ts_cad2cam, fovy, height, width, device=None, return_count=False):
    """``cad``: an .obj path or a (vertices, faces) pair; ``Ts_cad2cam``: 4 x 4 or [N, 4, 4].  Returns
    (None, depths float32 [N, H, W] with NaN off the model, masks bool [N, H, W]) as NumPy -- without the leading
    axis for a single 4 x 4 -- and with ``return_count`` the covered pixels per image (int32, = masks.sum)."""
    if isinstance(cad, (str, os.PathLike)):
        cad = mesh_sdf.load_obj(cad)
    Ts = np.asarray(Ts_cad2cam, np.float64)
    ndim = Ts.ndim
    if ndim == 2:
        Ts = Ts[None]
    if Ts.shape != (Ts.shape[0], 4, 4):
        raise ValueError("Ts_cad2cam must be 4 x 4 or [N, 4, 4]")
    n = Ts.shape[0]
    out = render_module.render_meshes([cad], Ts, fovy_intrinsics(fovy, height, width), height, width,
                                      targets=list(range(n)), mesh_index=[0] * n, device=device)
    depths = out["depth"].cpu().numpy()
    masks = out["instance"].cpu().numpy() >= 0
    count = out["count"].cpu().numpy()
    if n == 0:
        depths, masks = depths[:0], masks[:0]
    if ndim == 2:
        depths, masks, count = depths[0], masks[0], count[0]
    return (None, depths, masks, count) if return_count else (None, depths, masks)
