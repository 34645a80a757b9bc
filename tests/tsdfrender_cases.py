"""TEST INFRASTRUCTURE: the TSDF-render cases and their two runners -- the product (contrib.TsdfVolume.render /
InstanceTsdfVolume.render on a device, or on the host emulator) and the mirror (tests/tsdfrender_ref.py) -- whose
results the tests compare byte for byte: the summary, depth, end code, label image and ``sampled`` of every render.

A case is a volume ("plain": TsdfVolume, "instance": InstanceTsdfVolume) and a list of operations
  ("integrate", depth, K, T, label or None)
  ("poke", (k, j, i), tsdf, weight)          one voxel written directly
  ("render", K, T, options)                  options: step, max_steps (given: through the C entry point, the step cap),
                                             labels, min_count
and every render is run for each block edge asked for.  Images are 24 x 32.  The cases:
  a .. e   tsdf_cases' own (their integrates and ray-casts, the skipped integrate left out): the old volumes and poses;
           c and d, which have no ray-cast, get one from case a's pose after their last integrate.
  deep     tsdf_cases' scene (a plane at z = 1.1, a sphere in front of it) in a 24 x 19 x 26 volume of 4 cm from z = 0.5
           to 1.5: 31 cm of seen-free space in front of the sphere, 60 cm in front of the plane, 30 cm of unseen space
           behind it; n - 1 = 23, 18, 25, so the last block is clipped for every B.  Renders: a fresh volume (all
           UNKNOWN); after two integrates the main render from a third pose; steps of 0.15 and 0.25 m, beyond the
           truncation (a hit right after a FREE sample); from behind the plane (back faces); from 1 m to the side (rays
           that miss the box); the step cap at 3 and at 9 samples, inside a run; from behind the plane with a step of
           7 cm, which takes a ray from an UNKNOWN block over the half-seen cell straight to a valid sample behind the
           surface (a back face right after an UNKNOWN run; with the default step an invalid sample lies between).
  free     an 11 x 10 x 9 volume of 2 cm that one frame saw entirely free (every block FREE, every ray of a narrow camera LEFT);
           then a voxel with tsdf 1 and weight 0 and one with weight 1 and the float32 below 1 are written into it.
  labels   tsdflabel_cases' scene and volume (37 x 29 x 33 of 2 cm), three labelled frames, rendered with labels from
           the held-out pose with min_count 1 and 3 and with a step beyond the truncation; the step cap at 4.
"""
import numpy as np
import torch

import tsdf_cases as TC
import tsdf_ref as R
import tsdflabel_cases as LC
import tsdflabel_ref as LR
import tsdfrender_ref as RR
from morefusion_amd import _lib
from morefusion_amd.contrib import InstanceTsdfVolume, TsdfVolume

H, W = 24, 32
BLOCKS = (2, 4, 8)
K_WIDE = np.array([[30.0, 0, 15.3], [0, 29.0, 12.4], [0, 0, 1]])
K_NARROW = np.array([[300.0, 0, 15.5], [0, 300.0, 11.5], [0, 0, 1]])
DEEP_VOLUME = dict(dims=(24, 19, 26), pitch=0.04, origin=(-0.44, -0.36, 0.5), truncation=0.1)
FREE_VOLUME = dict(dims=(11, 10, 9), pitch=0.02, origin=(-0.08, -0.08, 0.55))
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
NAMES = ("a", "b", "c", "d", "e", "deep", "free", "labels")
MAIN = ("deep", 1)  # (case, index among its renders): the render the coverage thresholds are about


def make_case(name):
    """-> dict(kind, volume, ops)."""
    if name in "abcde":
        old = TC.make_case(name)
        ops = []
        for op in old["ops"]:
            if op[0] == "integrate":
                if not op[3]:  # (a set skip word changes nothing)
                    ops.append(("integrate", op[1], old["K"], op[2], None))
            else:
                ops.append(("render", old["K"], op[1], dict(max_steps=op[2])))
        if name in "cd":  # (no ray-cast of their own: the capped weight, the holes' unseen voxels)
            ops.append(("render", old["K"], TC.pose((-0.04, 0.06, -0.03), (-0.05, 0.04, 0.02)), {}))
        return dict(kind="plain", volume=old["volume"], ops=ops)
    if name == "deep":
        K = K_WIDE
        T0, T1 = TC.pose(), TC.pose((0.03, -0.05, 0.02), (0.06, -0.03, 0.05))
        T2 = TC.pose((-0.04, 0.06, -0.03), (-0.05, 0.04, 0.02))
        behind = np.diag([-1.0, 1.0, -1.0, 1.0])
        behind[2, 3] = 2.0
        ops = [("render", K, T0, {}),
               ("integrate", TC.render_scene(K, T0, H, W), K, T0, None),
               ("integrate", TC.render_scene(K, T1, H, W), K, T1, None),
               ("render", K, T2, {}), ("render", K, T2, dict(step=0.15)), ("render", K, T0, dict(step=0.25)),
               ("render", K, behind, {}), ("render", K, TC.pose(t=(1.0, 0.0, 0.0)), {}),
               ("render", K, T0, dict(max_steps=3)), ("render", K, T2, dict(max_steps=9)),
               ("render", K, behind, dict(step=0.07))]
        return dict(kind="plain", volume=DEEP_VOLUME, ops=ops)
    if name == "free":
        T0 = TC.pose()
        ops = [("integrate", TC.render_scene(K_WIDE, T0, H, W), K_WIDE, T0, None), ("render", K_NARROW, T0, {}),
               ("poke", (2, 6, 5), 1.0, 0.0), ("poke", (6, 1, 2), BELOW_ONE, 1.0), ("render", K_NARROW, T0, {})]
        return dict(kind="plain", volume=FREE_VOLUME, ops=ops)
    if name == "labels":
        ops = [(lambda d, l, T: ("integrate", d, LC.K, T, l))(*LC.frame(k)) for k in range(3)]
        ops += [("render", LC.K, LC.HELD_OUT, dict(labels=True)), ("render", LC.K, LC.HELD_OUT, dict(labels=True, min_count=3)),
                ("render", LC.K, LC.frame_pose(1), dict(labels=True, step=0.2)),
                ("render", LC.K, LC.HELD_OUT, dict(max_steps=4))]
        return dict(kind="instance", volume=LC.VOLUME, ops=ops)
    raise KeyError(name)


def fake_labels(dims, seed=0):
    """(label, count) pairs for a volume that has none: the label rule needs only an int32 array to look up."""
    nx, ny, nz = dims
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(-1, 5, (nz, ny, nx)), rs.randint(0, 4, (nz, ny, nx))], -1).astype(np.int32)


def run_mirror(case, blocks=BLOCKS, reference=False):
    """-> [per render: {B: tsdfrender_ref's dict, with the summary}].  With ``reference``
    every entry also holds "raycast" = tsdf_ref's (depth, code) of the same volume and arguments, and a plain volume is
    rendered with ``fake_labels`` so that the label rule is exercised on it too."""
    instance = case["kind"] == "instance"
    vol = (LR.InstanceVolume if instance else R.Volume)(**case["volume"])
    if reference and not instance:
        vol.labels = fake_labels(vol.dims)
    out = []
    for op in case["ops"]:
        if op[0] == "integrate":
            _, depth, K, T, label = op
            vol.integrate(depth, K, T, **({} if label is None else dict(label=label)))
        elif op[0] == "poke":
            vol.volume[op[1]] = (op[2], op[3])
        else:
            _, K, T, opt = op
            labels = opt.get("labels", False) or (reference and not instance)
            res = {B: RR.render_volume(vol, K, T, H, W, B, step=opt.get("step"), max_steps=opt.get("max_steps"),
                                       labels=labels, min_count=opt.get("min_count", 1)) for B in blocks}
            if reference:
                res["raycast"] = vol.raycast(K, T, H, W, step=opt.get("step"), max_steps=opt.get("max_steps"))
                res["labels"] = vol.labels
                res["args"] = (vol.origin, vol.pitch, K, T, opt.get("min_count", 1))
            out.append(res)
    return out


def render_capped(vol, K, T, B, max_steps, summary):
    """mf_tsdf_render with TsdfVolume.render's defaults and the given ``max_steps`` -> (depth, code, stats)."""
    T = torch.as_tensor(T).to(vol.device)
    depth = torch.full((H, W), -1.0, dtype=torch.float32, device=vol.device)
    code = torch.full((H, W), 255, dtype=torch.uint8, device=vol.device)
    stats = torch.full((H, W, 2), -1, dtype=torch.int32, device=vol.device)
    _lib.check(_lib.lib().mf_tsdf_render(
        _lib.ptr(vol.volume), *vol.dims, *vol.origin, vol.pitch, vol.truncation / 2.0, 0.0, float("inf"), max_steps, H,
        W, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), _lib.ptr(T), _lib.ptr(summary), B, None, 1,
        _lib.ptr(depth), _lib.ptr(code), None, _lib.ptr(stats), _lib.stream_ptr()), "mf_tsdf_render")
    return depth, code, stats


def run_product(case, device, blocks=BLOCKS):
    """The same through the product on tensors of ``device`` -> [per render: {B: dict(summary, depth, code, stats,
    label if asked for)}].  Poses alternate between NumPy arrays and device tensors, the summary between the one
    ``render`` makes itself and one from ``block_summary`` that is passed in."""
    instance = case["kind"] == "instance"
    vol = (InstanceTsdfVolume if instance else TsdfVolume)(device=device, **case["volume"])
    out = []
    for n, op in enumerate(case["ops"]):
        give = (lambda x: torch.as_tensor(x).to(device)) if n % 2 else (lambda x: x)  # noqa: E731
        if op[0] == "integrate":
            _, depth, K, T, label = op
            vol.integrate(give(depth), K, give(T), **({} if label is None else dict(label=give(label))))
        elif op[0] == "poke":
            vol.volume[op[1]] = torch.tensor([op[2], op[3]], dtype=torch.float32, device=device)
        else:
            _, K, T, opt = op
            res = {}
            for B in blocks:
                summary = vol.block_summary(B)
                if opt.get("max_steps") is not None:
                    depth, code, stats = render_capped(vol, K, T, B, opt["max_steps"], summary)
                    got = dict(depth=depth, code=code, stats=stats)
                else:
                    kw = dict(step=opt.get("step"), block=B, summary=summary if (n + B) % 4 else None,
                              return_code=True, return_stats=True)
                    if opt.get("labels"):
                        depth, label, code, stats = vol.render(K, give(T), H, W, labels=True,
                                                               min_count=opt.get("min_count", 1), **kw)
                        got = dict(depth=depth, code=code, stats=stats, label=label)
                    else:
                        depth, code, stats = vol.render(K, give(T), H, W, **kw)
                        got = dict(depth=depth, code=code, stats=stats)
                res[B] = {k: v.cpu().numpy() for k, v in dict(got, summary=summary).items()}
            out.append(res)
    return out


def assert_equal(got, exp, blocks=BLOCKS):
    """Summary, depth, code, label and stats[..., 0] bitwise; sampled <= visited <= the ray's samples."""
    assert len(got) == len(exp)
    for n, (g, e) in enumerate(zip(got, exp)):
        for B in blocks:
            for key in ("summary", "depth", "code", "label"):
                if key in g[B]:
                    assert g[B][key].dtype == e[B][key].dtype and g[B][key].shape == e[B][key].shape, (n, B, key)
                    assert g[B][key].tobytes() == e[B][key].tobytes(), (n, B, key, int((g[B][key] != e[B][key]).sum()))
            sampled, visited = g[B]["stats"][..., 0], g[B]["stats"][..., 1]
            assert g[B]["stats"].dtype == np.int32 and np.array_equal(sampled, e[B]["sampled"]), (n, B, "sampled")
            assert (sampled <= visited).all() and (visited <= e[B]["total"]).all(), (n, B, "visited")
