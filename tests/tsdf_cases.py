"""TEST INFRASTRUCTURE: the TSDF-fusion cases and their two runners -- the product (contrib.TsdfVolume on a device, or
on the host emulator) and the mirror (tests/tsdf_ref.py) -- whose results the tests compare with array_equal: the
volume's bytes after every integrate, depth and end code of every ray-cast.

A case is a volume, a camera and a list of operations ("integrate", depth, T, skip word or None) / ("raycast", T,
max_steps or None).  The scene is a plane z = 1.1 and a sphere in front of it, in the map frame, rendered analytically.
The smallest shapes that can still go wrong:
  a  volume 23 x 19 x 17 (no multiple of 64 or 256, three different sizes: a swapped stride shows), image 24 x 32; two
     integrates from different poses outside the box, a ray-cast from a third.
  b  identity rotation and an integer principal point: the centre column's rays have d_x = 0 and the centre row's
     d_y = 0 exactly.  Ray-casts with the camera's x inside the slab, outside it (those rays miss the box) and with
     the camera inside the volume.
  c  max_weight = 2 and the same frame integrated at three poses 1 cm apart: the weight stops at 2, the third update
     still moves the tsdf.
  d  holes as NaN, 0 and a negative depth; a camera inside the box (voxels behind it); voxels more than the truncation
     behind the surface; an integrate whose skip word is 2 (nothing changes) and one whose skip word is 0.
  e  a ray-cast from behind the plane (back faces, depth 0), one of a fresh volume (all zeros) and one with max_steps
     = 3 through the C entry point (the step cap; TsdfVolume.raycast's own max_steps cannot bind).

The model-tracking sequences (tests/test_tsdf_host.py, and the first seed on the device): 4 frames at 120 x 160 of
synthetic.make_tracking_sequence for the seeds of camtrack_cases.ACCURACY_SEEDS, default knobs, tracked from the
identity into MODEL_VOLUME.  MODEL_ERRORS holds what the mirror reaches: (translation error in m, rotation error in
rad) of frames 1, 2 and 3 (python tests/tsdf_cases.py prints them).
"""
import numpy as np
import torch

import camtrack_cases as CC
import camtrack_ref as CR
import tsdf_ref as R
from morefusion_amd import _lib
from morefusion_amd.contrib import TsdfVolume

PLANE_Z, SPHERE_C, SPHERE_R = 1.1, np.array([0.05, -0.02, 0.93]), 0.12

# the table scene of make_tracking_sequence: x in -0.8 .. 0.8, y in -0.62 .. 0.3, z in 0.3 .. 1.5 at 1 cm
MODEL_VOLUME = dict(dims=(161, 93, 121), pitch=0.01, origin=(-0.8, -0.62, 0.3))
MODEL_FRAMES = 4
# recorded from the mirror: {seed: ((t_err, r_err) of frame 1, of frame 2, of frame 3)}
MODEL_ERRORS = {
    0: ((1.115e-3, 9.230e-4), (9.166e-4, 6.090e-4), (7.503e-4, 6.157e-4)),
    1: ((8.623e-4, 1.863e-3), (7.774e-4, 1.710e-3), (7.564e-4, 1.704e-3)),
    3: ((2.578e-4, 3.954e-4), (3.769e-4, 3.329e-4), (4.253e-5, 8.678e-5)),
}


def rotation(rx, ry, rz):
    """A small rotation: the matrix of the normalised quaternion (1, rx / 2, ry / 2, rz / 2)."""
    return CR.quat_matrix(CR.quat_normalise([1.0, rx / 2.0, ry / 2.0, rz / 2.0]))


def pose(rot=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(*rot), t
    return T


def render_scene(K, T, H, W):
    """The plane and the sphere seen from T_sensor_to_map = T -> float32 [H, W] depth along the camera's z, NaN where
    nothing is hit."""
    v, u = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(all="ignore"):
        t_plane = np.where(d[..., 2] > 0, (PLANE_Z - o[2]) / d[..., 2], np.inf)
        c = SPHERE_C - o
        b, dd = (d * c).sum(-1), (d * d).sum(-1)
        disc = b * b - dd * (c @ c - SPHERE_R ** 2)
        t_sphere = np.where(disc >= 0, (b - np.sqrt(disc)) / dd, np.inf)
    t = np.minimum(np.where(t_plane > 0, t_plane, np.inf), np.where(t_sphere > 0, t_sphere, np.inf))
    return np.where(np.isfinite(t), t, np.nan).astype(np.float32)


def make_case(name):
    """-> dict(volume (TsdfVolume's arguments), K, H, W, ops)."""
    H, W = 24, 32
    volume = dict(dims=(23, 19, 17), pitch=0.04, origin=(-0.44, -0.36, 0.6), truncation=0.1)
    K = np.array([[30.0, 0, 15.3], [0, 29.0, 12.4], [0, 0, 1]])
    if name == "a":
        T0, T1 = pose(), pose((0.03, -0.05, 0.02), (0.06, -0.03, 0.05))
        T2 = pose((-0.04, 0.06, -0.03), (-0.05, 0.04, 0.02))
        ops = [("integrate", render_scene(K, T0, H, W), T0, None), ("integrate", render_scene(K, T1, H, W), T1, None),
               ("raycast", T2, None)]
    elif name == "b":
        K = np.array([[30.0, 0, 16.0], [0, 29.0, 12.0], [0, 0, 1]])
        T0 = pose()
        ops = [("integrate", render_scene(K, T0, H, W), T0, None), ("raycast", T0, None),
               ("raycast", pose(t=(1.0, 0.0, 0.0)), None), ("raycast", pose(t=(0.02, -0.01, 0.7)), None)]
    elif name == "c":
        volume["max_weight"] = 2.0
        depth = render_scene(K, pose(), H, W)
        ops = [("integrate", depth, pose(t=(0.0, 0.0, 0.01 * k)), None) for k in range(3)]
    elif name == "d":
        T0, Tin = pose(), pose((0.0, 0.02, 0.0), (0.02, -0.01, 0.75))
        depth = render_scene(K, T0, H, W)
        depth[3:6, 4:9], depth[10, 11:14], depth[15:17, 20] = np.nan, 0.0, -0.5
        ops = [("integrate", depth, T0, None), ("integrate", render_scene(K, Tin, H, W), Tin, 2),
               ("integrate", render_scene(K, Tin, H, W), Tin, 0)]
    elif name == "e":
        T0 = pose()
        behind = np.diag([-1.0, 1.0, -1.0, 1.0])  # half a turn about y, from z = 2 back towards the plane
        behind[2, 3] = 2.0
        ops = [("raycast", T0, None), ("integrate", render_scene(K, T0, H, W), T0, None), ("raycast", behind, None),
               ("raycast", T0, 3)]
    else:
        raise KeyError(name)
    return dict(volume=volume, K=K, H=H, W=W, ops=ops)


def run_mirror(case):
    """-> [result per operation]: dict(volume, outcome) of an integrate, dict(depth, code) of a ray-cast."""
    vol, out = R.Volume(**case["volume"]), []
    for op in case["ops"]:
        if op[0] == "integrate":
            outcome = vol.integrate(op[1], case["K"], op[2], skip=op[3] or 0)
            out.append(dict(volume=vol.volume.copy(), outcome=outcome))
        else:
            depth, code = vol.raycast(case["K"], op[1], case["H"], case["W"], max_steps=op[2])
            out.append(dict(depth=depth, code=code))
    return out


def raycast_capped(vol, K, T, H, W, max_steps):
    """mf_tsdf_raycast with TsdfVolume.raycast's defaults and the given ``max_steps``."""
    T = torch.as_tensor(T).to(vol.device)
    depth = torch.full((H, W), -1.0, dtype=torch.float32, device=vol.device)
    code = torch.full((H, W), 255, dtype=torch.uint8, device=vol.device)
    _lib.check(_lib.lib().mf_tsdf_raycast(
        _lib.ptr(vol.volume), *vol.dims, *vol.origin, vol.pitch, vol.truncation / 2.0, 0.0, float("inf"), max_steps, H,
        W, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), _lib.ptr(T), _lib.ptr(depth), _lib.ptr(code),
        _lib.stream_ptr()), "mf_tsdf_raycast")
    return depth, code


def run_product(case, device):
    """The same through contrib.TsdfVolume on tensors of ``device``; poses and depths alternate between NumPy arrays
    and device tensors."""
    vol, out = TsdfVolume(device=device, **case["volume"]), []
    for n, op in enumerate(case["ops"]):
        give = (lambda x: torch.as_tensor(x).to(device)) if n % 2 else (lambda x: x)  # noqa: E731
        if op[0] == "integrate":
            skip = None if op[3] is None else torch.tensor([op[3]], dtype=torch.int32, device=device)
            vol.integrate(give(op[1]), case["K"], give(op[2]), skip_if=skip)
            out.append(dict(volume=vol.volume.cpu().numpy().copy()))
        else:
            if op[2] is None:
                depth, code = vol.raycast(case["K"], give(op[1]), case["H"], case["W"], return_code=True)
            else:
                depth, code = raycast_capped(vol, case["K"], op[1], case["H"], case["W"], op[2])
            out.append(dict(depth=depth.cpu().numpy(), code=code.cpu().numpy()))
    assert np.array_equal(vol.tsdf.cpu().numpy(), vol.volume.cpu().numpy()[..., 0])
    assert np.array_equal(vol.weight.cpu().numpy(), vol.volume.cpu().numpy()[..., 1])
    return out


def assert_equal(got, exp):
    assert len(got) == len(exp)
    for n, (g, e) in enumerate(zip(got, exp)):
        for key in ("volume", "depth", "code"):
            if key in e:
                assert g[key].dtype == e[key].dtype and g[key].shape == e[key].shape, (n, key)
                assert np.array_equal(g[key], e[key]), (n, key, int((g[key] != e[key]).sum()))


def coverage(results):
    """-> (the ray end codes, the integrate outcomes) that occur in a list of mirror results."""
    codes, outcomes = set(), set()
    for r in results:
        codes |= set(np.unique(r["code"]).tolist()) if "code" in r else set()
        outcomes |= set(np.unique(r["outcome"]).tolist()) if "outcome" in r else set()
    return codes, outcomes


def model_sequence(seed, height=CC.ACCURACY_SHAPE[0], width=CC.ACCURACY_SHAPE[1]):
    return CC.sequence(seed, MODEL_FRAMES, height, width)


def track_model_mirror(frames, volume=None, **knobs):
    """-> (poses [n, 4, 4], the mirror's ModelTracker)."""
    H, W = frames[0]["depth"].shape
    trk = R.ModelTracker(frames[0]["K"], H, W, R.Volume(**(volume or MODEL_VOLUME)), **knobs)
    return np.stack([trk.track(f["depth"]) for f in frames]), trk


if __name__ == "__main__":
    for seed in CC.ACCURACY_SEEDS:
        frames = model_sequence(seed)
        poses, trk = track_model_mirror(frames)
        print(seed, [tuple(float(f"{x:.3e}") for x in e) for e in CC.sequence_errors(frames, poses)], trk.status)
