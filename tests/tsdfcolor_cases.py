"""TEST INFRASTRUCTURE: the TSDF-colour cases and their two runners -- the product (contrib.TsdfVolume(colors=True) /
contrib.InstanceTsdfVolume(colors=True) on a device, or on the host emulator) and the mirror (tests/tsdfcolor_ref.py) --
whose results the tests compare with array_equal: the bytes of ``colors``, of the volume and of the labels after every
integrate, every colour image, and every set of sampled colours (mesh vertices, hand-placed points).

The scene, volume, camera and poses are those of tests/tsdflabel_cases.py: the ground plane z = 0 and two spheres seen
from 1.1 m above, a 37 x 29 x 33 volume of 2 cm voxels (35409: the last workgroup is partial, the three sizes differ),
24 x 32 images.  The scene is coloured analytically, as a function of the map-frame point a pixel sees: a smooth ramp
on the ground (red along x, green along y), one tint per sphere with a vertical shade, quantised to uint8.

A case is a list of operations:
  ("integrate", depth, T, label or None, skip word or None, color or None)
  ("color_image", T)        ray-cast from T, then the colours under that render
  ("mesh",)                 extract_mesh(colors=True): the vertices and their colours
  ("sample", points)
The sequences:
  a  three coloured frames; the colour image from a held-out pose; the mesh's vertex colours; hand-placed points
     (outside the box, on the last lattice plane and just inside it, on the first plane, in a cell with no coloured
     corner, in a cell with exactly one, a NaN)
  b  max_weight = 2 and four frames: the colour weight saturates
  c  holes in the depth and the colour of a frame whose skip word is set: the colours do not change
  d  color=None frames between coloured ones: the tsdf moves, the colours do not
  e  InstanceTsdfVolume(colors=True) fed labels and colours together"""
import numpy as np
import torch

import tsdfcolor_ref as CR
import tsdflabel_cases as LC
import tsdfmesh_ref as MR
from morefusion_amd.contrib import InstanceTsdfVolume, TsdfVolume

H, W, K, VOLUME, HELD_OUT = LC.H, LC.W, LC.K, LC.VOLUME, LC.HELD_OUT
TINTS = {1: (210.0, 60.0, 50.0), 3: (40.0, 90.0, 220.0)}


def analytic_color(depth, label, T):
    """The scene's colour at the map point every pixel sees (``depth``, ``label`` of LC.render from T) -> uint8
    [H, W, 3]."""
    v, u = np.mgrid[:H, :W].astype(np.float64)
    d = depth.astype(np.float64)
    p = np.stack([(u - K[0, 2]) / K[0, 0] * d, (v - K[1, 2]) / K[1, 1] * d, d], -1)
    m = p @ T[:3, :3].T + T[:3, 3]
    ground = np.stack([60.0 + 150.0 * (m[..., 0] + 0.4), 80.0 + 160.0 * (m[..., 1] + 0.3), np.full((H, W), 40.0)], -1)
    out = ground
    for i, tint in TINTS.items():
        shade = 0.8 + m[..., 2:3]  # brighter towards the top
        out = np.where((label == i)[..., None], np.asarray(tint) * shade, out)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def frame(k, **kw):
    """-> (depth, label, color, T) of frame k: LC.frame's depth and label, the colour of the scene as rendered."""
    depth, label, T = LC.frame(k, **kw)
    clean_depth, clean_label = LC.render(T)
    return depth, label, analytic_color(clean_depth, clean_label, T), T


def _exactly_on(o, pitch, n):
    """x with (x - o) / pitch == n exactly in float64."""
    x = o + pitch * n
    for _ in range(8):
        g = (x - o) / pitch
        if g == n:
            return x
        x = np.nextafter(x, -np.inf if g > n else np.inf)
    raise AssertionError("no float64 lands on the lattice plane")


def hand_points():
    """-> (points float64 [N, 3], names): see the module's text.  ``one corner`` was found on the mirror's sequence (a)
    (tests/test_tsdfcolor_host.py checks that it still is what its name says)."""
    o, p, (nx, ny, nz) = VOLUME["origin"], VOLUME["pitch"], VOLUME["dims"]
    last_x = _exactly_on(o[0], p, nx - 1)
    pts = [
        ("outside", (1.0, 0.0, 0.0)),
        ("below", (0.0, 0.0, o[2] - 0.001)),
        ("last plane", (last_x, 0.005, 0.003)),
        ("inside last cell", (last_x - 0.25 * p, 0.005, 0.003)),
        ("first plane", (_exactly_on(o[0], p, 0), 0.005, 0.003)),
        ("no corner", (0.003, 0.004, 0.45)),
        ("one corner", ONE_CORNER),
        ("ground", (0.013, -0.171, 0.004)),
        ("sphere 1", (-0.12, 0.02, 0.268)),
        ("nan", (np.nan, 0.0, 0.0)),
    ]
    return np.array([q for _, q in pts], np.float64), [n for n, _ in pts]


ONE_CORNER = (0.191, -0.111, 0.141)


def make_case(name):
    """-> dict(volume (the volume's arguments), instance (bool: InstanceTsdfVolume), ops)."""
    volume = dict(VOLUME)

    def integrate(k, skip=None, color=True, label=False):
        depth, lab, rgb, T = frame(k)
        return ("integrate", depth, T, lab if label else None, skip, rgb if color else None)

    if name == "a":
        ops = [integrate(0), integrate(1), integrate(2), ("color_image", HELD_OUT), ("mesh",),
               ("sample", hand_points()[0])]
    elif name == "b":
        volume["max_weight"] = 2.0
        ops = [integrate(k) for k in range(4)] + [("color_image", HELD_OUT)]
    elif name == "c":
        depth, _, rgb, T = frame(0)
        depth[3:6, 4:9], depth[10, 11:14], depth[15:17, 20] = np.nan, 0.0, -0.5
        ops = [("integrate", depth, T, None, None, rgb), integrate(1, skip=2), ("color_image", LC.frame_pose(1)),
               integrate(1, skip=0), ("color_image", np.diag([1.0, 1.0, 1.0, 1.0]))]  # (that pose looks away)
    elif name == "d":
        ops = [integrate(0), integrate(1, color=False), integrate(2), integrate(3, color=False, skip=0),
               ("color_image", HELD_OUT)]
    elif name == "e":
        ops = [integrate(0, label=True), integrate(1, label=True), integrate(2, label=True, color=False),
               integrate(3, color=True), integrate(4, label=True, skip=1), ("color_image", HELD_OUT), ("mesh",)]
    else:
        raise KeyError(name)
    return dict(volume=volume, instance=name == "e", ops=ops)


CASES = "abcde"


def run_mirror(case):
    """-> [result per operation]: dicts of arrays; an integrate's also holds ``what`` (tsdfcolor_ref's outcome per
    voxel) if the frame had a colour."""
    vol, out = CR.ColorVolume(**case["volume"]), []
    for op in case["ops"]:
        if op[0] == "integrate":
            _, depth, T, label, skip, color = op
            what = vol.integrate(depth, K, T, label=label, skip=skip or 0, color=color)
            res = dict(volume=vol.volume.copy(), colors=vol.colors.copy())
            if case["instance"]:
                res["labels"] = vol.labels.copy()
            out.append(dict(res, what=what) if color is not None else res)
        elif op[0] == "color_image":
            depth, _ = vol.raycast(K, op[1], H, W)
            out.append(dict(depth=depth, color_image=vol.color_image(depth, K, op[1])))
        elif op[0] == "mesh":
            vertices = MR.mesh(vol.volume, vol.origin, vol.pitch)["vertices"]
            out.append(dict(vertices=vertices, vertex_colors=vol.sample_colors(vertices)))
        else:
            out.append(dict(sampled=vol.sample_colors(op[1])))
    return out


def run_product(case, device):
    """The same through the product's classes on tensors of ``device``; poses, depths, labels, colours and points
    alternate between NumPy arrays and device tensors."""
    cls = InstanceTsdfVolume if case["instance"] else TsdfVolume
    vol, out = cls(device=device, colors=True, **case["volume"]), []
    for n, op in enumerate(case["ops"]):
        give = (lambda x: torch.as_tensor(x).to(device)) if n % 2 else (lambda x: x)  # noqa: E731
        if op[0] == "integrate":
            _, depth, T, label, skip, color = op
            skip = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=device)
            kw = {} if label is None else dict(label=give(label))
            vol.integrate(give(depth), K, give(T), skip_if=skip, color=None if color is None else give(color), **kw)
            res = dict(volume=vol.volume.cpu().numpy().copy(), colors=vol.colors.cpu().numpy().copy())
            if case["instance"]:
                res["labels"] = vol.labels.cpu().numpy().copy()
            out.append(res)
        elif op[0] == "color_image":
            depth = vol.raycast(K, give(op[1]), H, W)
            image = vol.color_image(depth if n % 2 else depth.cpu().numpy(), K, give(op[1]))
            out.append(dict(depth=depth.cpu().numpy(), color_image=image.cpu().numpy()))
        elif op[0] == "mesh":
            vertices, _, colors = vol.extract_mesh(colors=True)
            out.append(dict(vertices=vertices.cpu().numpy(), vertex_colors=colors.cpu().numpy()))
        else:
            out.append(dict(sampled=vol.sample_colors(give(op[1])).cpu().numpy()))
    return out


TRACKER_KNOBS = dict(levels=1, iterations=(6,), min_pairs=30)  # 24 x 32 images: a second level has too few pairs


def tracked_and_by_hand(device):
    """The five case frames through ModelTracker.track(depth, label, color) into an InstanceTsdfVolume(colors=True), and
    the same frames integrated by hand at the poses the tracker returned (a frame it lost left out)
    -> (the tracker's volume, the volume made by hand, the tracker, [lost per frame])."""
    from morefusion_amd.contrib import ModelTracker
    frames = [frame(k) for k in range(5)]
    vol = InstanceTsdfVolume(device=device, colors=True, **VOLUME)
    trk = ModelTracker(K, H, W, vol, T_first=frames[0][3], **TRACKER_KNOBS)
    poses, lost = [], []
    for k, (depth, label, rgb, _) in enumerate(frames):
        give = (lambda x: torch.as_tensor(x).to(device)) if k % 2 else (lambda x: x)  # noqa: E731
        poses.append(trk.track(give(depth), give(label), give(rgb)))
        lost.append(k > 0 and trk.lost)
    by_hand = InstanceTsdfVolume(device=device, colors=True, **VOLUME)
    for (depth, label, rgb, _), T, gone in zip(frames, poses, lost):
        if not gone:
            by_hand.integrate(depth, K, T, label=label, color=rgb)
    return vol, by_hand, trk, lost


KEYS = ("volume", "colors", "labels", "depth", "color_image", "vertices", "vertex_colors", "sampled")


def assert_equal(got, exp):
    assert len(got) == len(exp)
    for n, (g, e) in enumerate(zip(got, exp)):
        assert set(g) == set(e) - {"what"}, (n, sorted(g), sorted(e))
        for key in g:
            assert key in KEYS
            assert g[key].dtype == e[key].dtype and g[key].shape == e[key].shape, \
                (n, key, g[key].dtype, e[key].dtype, g[key].shape, e[key].shape)
            assert np.array_equal(g[key], e[key], equal_nan=g[key].dtype.kind == "f"), \
                (n, key, int((g[key] != e[key]).sum()))
