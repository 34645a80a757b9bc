"""TEST INFRASTRUCTURE: the TSDF-label cases and their two runners -- the product (contrib.InstanceTsdfVolume on a
device, or on the host emulator) and the mirror (tests/tsdflabel_ref.py) -- whose results the tests compare with
array_equal: the bytes of ``labels`` and of the volume after every integrate, every label image, statistics table and
its map-frame form, and the grids and origins of every publication.

The scene, in a map frame with z up: the ground plane z = 0 labelled -1 and two spheres above it with the ids 1 and 3,
seen by a camera 1.1 m above the ground that looks down, rendered analytically (depth and label) from poses a few
centimetres and degrees apart.  The volume is 37 x 29 x 33 voxels of 2 cm: 35409 voxels, no multiple of 256 (the last
workgroup is partial), three different sizes (a swapped stride shows), reaching 9 cm below the ground.  Images 24 x 32.
The label images that are fused carry what a tracker's output carries: a stripe of -2 ("uncertain"), pixels of 0 and -5
(no votes), and in frame 0 a patch of id 7 on the ground that no later frame confirms.

A case is a list of operations:
  ("integrate", depth, T, label or None, skip word or None)
  ("label_image", T, min_count)            ray-cast from T, then the labels under that render
  ("stats", ids, min_weight, min_count)
  ("publish", T, ids, pitches, centers or None, dim, keyword arguments)
The sequences:
  a  three frames with consistent labels; statistics after frame 0 (id 7 is there) and at the end over [1, 3, 7, 9]
     (7 released, 9 never seen: empty rows) and over 64 ids; the label image from a held-out pose; every publication.
  b  max_count = 2 and four frames: the count saturates.
  c  five frames, the two spheres' labels swapped from frame 2 on: counts fall, reach 0, voxels are re-claimed.
  d  holes in the depth (NaN, 0, negative) and a frame whose skip word is set: neither tensor changes.
  e  label=None frames between labelled ones: the tsdf moves, the labels do not.
The publications (each with D = 8 and D = 32): a grid that straddles the volume's border; ground_z = 0 with a grid
that reaches below the plane; free_as_noentry on and off with min_count 1 and 2 from a pose turned about all three axes,
centres given and centres taken from the statistics."""
import numpy as np
import torch

import tsdf_cases as TC
import tsdflabel_ref as LR
from morefusion_amd.contrib import InstanceTsdfVolume

H, W = 24, 32
K = np.array([[30.0, 0, 15.3], [0, 29.0, 12.4], [0, 0, 1]])
VOLUME = dict(dims=(37, 29, 33), pitch=0.02, origin=(-0.36, -0.28, -0.09))
SPHERES = ((1, np.array([-0.12, 0.02, 0.17]), 0.10), (3, np.array([0.13, -0.03, 0.20]), 0.09))
DOWN = np.array([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 1.1], [0, 0, 0, 1]])  # 1.1 m up, looking down
IDS = [1, 3, 7, 9]
IDS_64 = [-1] + list(range(1, 64))
HELD_OUT = DOWN @ TC.pose((0.05, 0.04, -0.06), (-0.03, 0.04, 0.02))


def frame_pose(k):
    rot = [(0.0, 0.0, 0.0), (0.04, -0.05, 0.03), (-0.05, 0.03, -0.04), (0.03, 0.05, 0.05), (-0.03, -0.04, 0.02)][k]
    t = [(0.0, 0.0, 0.0), (0.04, -0.03, 0.02), (-0.05, 0.03, 0.01), (0.03, 0.04, -0.02), (-0.02, -0.05, 0.03)][k]
    return DOWN @ TC.pose(rot, t)


def render(T, swap=False):
    """The scene from T_sensor_to_map = T -> (depth float32 [H, W] along the camera's z, label int32 [H, W]): the
    analytic render, every pixel sees the ground or a sphere.  ``swap``: the spheres carry each other's id."""
    v, u = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(all="ignore"):
        best = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)  # the plane z = 0
        label = np.full((H, W), -1, np.int32)
        for (i, c, r), shown in zip(SPHERES, (3, 1) if swap else (1, 3)):
            oc = c - o
            b, dd = (d * oc).sum(-1), (d * d).sum(-1)
            disc = b * b - dd * (oc @ oc - r ** 2)
            t = np.where(disc >= 0, (b - np.sqrt(disc)) / dd, np.inf)
            nearer = (t > 0) & (t < best)
            best, label = np.where(nearer, t, best), np.where(nearer, shown, label).astype(np.int32)
    assert np.isfinite(best).all()
    return best.astype(np.float32), label


def frame(k, swap=False, tracker_noise=True):
    """-> (depth, label, T) of frame k; the label with what a tracker's output carries (see the module's text)."""
    T = frame_pose(k)
    depth, label = render(T, swap)
    if tracker_noise:
        label[:, 9 + k] = -2
        label[2, 3:6], label[20, 25:28] = 0, -5
        if k == 0:
            label[17:21, 14:18] = 7  # on the ground between the spheres, in this frame alone
    return depth, label, T


def publications():
    turned = DOWN @ TC.pose((0.2, -0.15, 0.3), (0.05, -0.04, 0.03))
    ops = []
    for dim, pitch in ((8, 0.03), (32, 0.012)):
        p = [pitch, 0.75 * pitch]
        border = [[-0.34, 0.02, 0.17], [0.13, -0.27, 0.5]]
        ops.append(("publish", frame_pose(1), [1, 3], p, border, dim, {}))
        ops.append(("publish", frame_pose(2), [1, 3], p, [[-0.12, 0.02, 0.05], [0.13, -0.03, 0.02]], dim,
                    dict(ground_z=0.0)))
        for min_count in (1, 2):
            for free in (True, False):
                centers = None if (min_count == 1) == free else [[-0.12, 0.02, 0.12], [0.13, -0.03, 0.15]]
                ops.append(("publish", turned, [1, 3], p, centers, dim,
                            dict(min_count=min_count, free_as_noentry=free, empty_above=0.25)))
    ops.append(("publish", turned, [1, 3, 9], [0.03, 0.03, 0.03], None, 8, {}))  # 9 has no voxel: dropped
    return ops


def make_case(name):
    """-> dict(volume (InstanceTsdfVolume's arguments), ops)."""
    volume = dict(VOLUME)
    integrate = lambda k, skip=None, **kw: (lambda d, l, T: ("integrate", d, T, l, skip))(*frame(k, **kw))  # noqa: E731
    if name == "a":
        ops = [integrate(0), ("stats", IDS, 1.0, 1), integrate(1), integrate(2), ("stats", IDS, 1.0, 1),
               ("stats", IDS, 2.0, 2), ("stats", IDS_64, 1.0, 1), ("label_image", HELD_OUT, 1),
               ("label_image", HELD_OUT, 3)] + publications()
    elif name == "b":
        volume["max_count"] = 2
        ops = [integrate(k) for k in range(4)] + [("stats", IDS, 1.0, 2)]
    elif name == "c":
        ops = [integrate(k, swap=k >= 2) for k in range(5)] + [("stats", IDS, 1.0, 1), ("label_image", HELD_OUT, 1)]
    elif name == "d":
        depth, label, T = frame(0)
        depth[3:6, 4:9], depth[10, 11:14], depth[15:17, 20] = np.nan, 0.0, -0.5
        ops = [("integrate", depth, T, label, None), integrate(1, skip=2), ("label_image", frame_pose(1), 1),
               integrate(1, skip=0), ("label_image", np.diag([1.0, 1.0, 1.0, 1.0]), 1)]  # (that pose looks away)
    elif name == "e":
        d1, _, T1 = frame(1)
        d3, _, T3 = frame(3)
        ops = [integrate(0), ("integrate", d1, T1, None, None), integrate(2), ("integrate", d3, T3, None, 0),
               ("stats", IDS, 1.0, 1)]
    else:
        raise KeyError(name)
    return dict(volume=volume, ops=ops)


CASES = "abcde"


def _publish_result(out):
    return {k: (np.asarray(v) if isinstance(v, (list, np.ndarray)) else v.cpu().numpy()) for k, v in out.items()}


def run_mirror(case):
    """-> [result per operation]: dicts of arrays; the mirror's also hold ``vote`` / ``outcome`` for the coverage."""
    vol, out = LR.InstanceVolume(**case["volume"]), []
    for op in case["ops"]:
        if op[0] == "integrate":
            _, depth, T, label, skip = op
            vote = vol.integrate(depth, K, T, label=label, skip=skip or 0)
            res = dict(volume=vol.volume.copy(), labels=vol.labels.copy())
            out.append(dict(res, vote=vote) if label is not None else res)
        elif op[0] == "label_image":
            depth, _ = vol.raycast(K, op[1], H, W)
            out.append(dict(depth=depth, label_image=vol.label_image(depth, K, op[1], op[2])))
        elif op[0] == "stats":
            table = vol.instance_table(op[1], op[2], op[3])
            out.append(dict(table=table, **LR.stats_in_map_frame(table, vol.origin, vol.pitch)))
        else:
            _, T, ids, pitch, centers, dim, kw = op
            classes = [10 + i for i in ids]
            if centers is None:
                stats = vol.instance_stats(ids, kw.get("min_weight", 1.0), kw.get("min_count", 1))
                keep = np.flatnonzero(stats["count"] > 0)
                ids, pitch, classes = ([x[n] for n in keep] for x in (ids, pitch, classes))
                centers = stats["center"][keep]
            res = vol.publish_grids(T, ids, pitch, centers, dim=dim, **kw)
            res["grid_nontarget_empty"] = res["grid_nontarget_empty"].astype(bool)
            out.append(dict(res, instance_ids=np.asarray(ids), class_ids=np.asarray(classes),
                            pitch=np.asarray(pitch, np.float32)))
    return out


def run_product(case, device):
    """The same through contrib.InstanceTsdfVolume on tensors of ``device``; poses, depths and labels alternate
    between NumPy arrays and device tensors."""
    vol, out = InstanceTsdfVolume(device=device, **case["volume"]), []
    for n, op in enumerate(case["ops"]):
        give = (lambda x: torch.as_tensor(x).to(device)) if n % 2 else (lambda x: x)  # noqa: E731
        if op[0] == "integrate":
            _, depth, T, label, skip = op
            skip = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=device)
            vol.integrate(give(depth), K, give(T), label=None if label is None else give(label), skip_if=skip)
            out.append(dict(volume=vol.volume.cpu().numpy().copy(), labels=vol.labels.cpu().numpy().copy()))
        elif op[0] == "label_image":
            depth = vol.raycast(K, give(op[1]), H, W)
            image = vol.label_image(depth if n % 2 else depth.cpu().numpy(), K, give(op[1]), min_count=op[2])
            out.append(dict(depth=depth.cpu().numpy(), label_image=image.cpu().numpy()))
        elif op[0] == "stats":
            table = vol.instance_table(op[1], op[2], op[3]).cpu().numpy()
            out.append(dict(table=table, **vol.instance_stats(op[1], min_weight=op[2], min_count=op[3])))
        else:
            _, T, ids, pitch, centers, dim, kw = op
            classes = {i: 10 + i for i in ids} if n % 2 else [10 + i for i in ids]
            res = vol.publish_grids(give(T), ids, pitch, centers=centers, class_ids=classes, dim=dim, **kw)
            out.append(_publish_result(res))
    return out


KEYS = ("volume", "labels", "depth", "label_image", "table", "count", "center", "bbx_min", "bbx_max", "instance_ids",
        "class_ids", "pitch", "origin", "grid_target", "grid_noentry", "grid_nontarget_empty")


def assert_equal(got, exp):
    assert len(got) == len(exp)
    for n, (g, e) in enumerate(zip(got, exp)):
        assert set(g) == set(e) - {"vote", "outcome"}, (n, sorted(g), sorted(e))
        for key in g:
            assert key in KEYS
            assert g[key].dtype == e[key].dtype and g[key].shape == e[key].shape, (n, key, g[key].dtype, e[key].dtype)
            assert np.array_equal(g[key], e[key], equal_nan=g[key].dtype.kind == "f"), \
                (n, key, int((g[key] != e[key]).sum()))


def coverage(results):
    """-> (the votes, the publish outcomes) that occur in a list of mirror results."""
    votes, outcomes = set(), set()
    for r in results:
        votes |= set(np.unique(r["vote"]).tolist()) if "vote" in r else set()
        outcomes |= set(np.unique(r["outcome"]).tolist()) if "outcome" in r else set()
    return votes, outcomes
