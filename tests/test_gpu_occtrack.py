"""Instance tracking on the MI355X (csrc/occtrack.hip through contrib.InstanceTracker) against the mirror
(tests/occtrack_ref.py) bit for bit: the two-frame scenario of tests/occtrack_cases.py at 121 x 163 (odd in both
directions: the 2 x 2 splat clips at row / column 0 and the last stride-2 pixel is the last pixel) with 5 instances,
run-to-run identity, NumPy and device inputs; a 480 x 640 pair of label images with 8 instances whose components and
bands cross workgroup tiles; the overlap pass on both of its paths (3 x 3 ids: LDS bins, 40 x 40: global atomics); a
three-frame sequence with a moving sensor; and the multi-view example end to end (its own process and time limit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import occtrack_cases as C
import occtrack_ref as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

from morefusion_amd import _lib, synthetic  # noqa: E402
from morefusion_amd.contrib import track_instance_ids  # noqa: E402

# small images: the reference's thresholds would veto every object; these keep objects of >= 6 pixels across
THRESHOLDS = dict(min_mask=5, min_bbox=8, min_side=6, min_area=16, band=2, iou=0.4, coverage=0.9)
SEED_TWO_FRAMES, SEED_SEQUENCE = 0, 0


@pytest.fixture(scope="module")
def scenario():
    return C.make_scenario(SEED_TWO_FRAMES, 121, 163, 5, THRESHOLDS)


@pytest.fixture(scope="module")
def product(scenario):
    return C.run_product(scenario, "cuda")


@pytest.fixture(scope="module")
def mirror(scenario, product):
    return C.run_mirror(scenario, product[0]["boxes"])


def test_two_frames_bitwise_vs_mirror(scenario, product, mirror):
    (got, m, _), (exp, ref) = product, mirror
    C.check_cases(scenario, exp)
    assert np.array_equal(got["frame0"]["label_tracked"], exp["frame0"]["label_tracked"])
    C.check_frame1(got, exp)
    rendered = exp["frame1"]["label_rendered"]
    assert (rendered[0] >= 0).any() or (rendered[:, 0] >= 0).any() or (rendered[-1] >= 0).any()  # a clipped splat
    C.logodds_equal(m, ref)
    assert int(m._overflow[0]) == 0


def test_run_to_run_identity(scenario, product):
    again = C.run_product(scenario, "cuda")[0]
    for frame in ("frame0", "frame1"):
        for k, v in product[0][frame].items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, again[frame][k], equal_nan=v.dtype.kind == "f"), (frame, k)


def _label_pair(H, W, n, seed):
    """Two label images of n rectangles each: the detection is the reference shifted by a few pixels, its ids
    permuted, plus specks; one reference rectangle is wider than a workgroup's 256 pixels."""
    rs = np.random.RandomState(seed)
    ref = np.full((H, W), -2, np.int32)
    det = np.full((H, W), -1, np.int32)
    perm = rs.permutation(n)
    rows = np.linspace(0.12 * H, 0.88 * H, n + 1).astype(int)
    for k in range(n):
        r0, r1 = rows[k] + 2, rows[k + 1] - 2
        c0 = int(rs.uniform(0.12, 0.3) * W)
        c1 = c0 + (int(0.55 * W) if k == 0 else int(rs.uniform(0.15, 0.4) * W))
        ref[r0:r1, c0:c1] = k + 1
        dr, dc = rs.randint(-2, 3), rs.randint(-6, 7)
        det[max(r0 + dr, 0):r1 + dr, max(c0 + dc, 0):c1 + dc] = perm[k]
    for _ in range(6 * n):  # specks: components below min_area
        j, i, k = rs.randint(0, H - 3), rs.randint(0, W - 3), rs.randint(0, n)
        ref[j:j + 2, i:i + 3] = k + 1
        det[j + 1:j + 3, i:i + 2] = perm[k]
    return ref, det


def _track_on_device(ref, det, ref_ids, det_ids, counter, thresholds):
    c = torch.tensor([counter], dtype=torch.int32).cuda()
    out = track_instance_ids(torch.as_tensor(ref).cuda(), torch.as_tensor(det).cuda(), ref_ids, det_ids, c, thresholds)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check_track(got, exp, ref_ids, det_ids):
    assert dict(zip(det_ids, got["remap"][:-1].tolist())) == exp["remap"]
    assert int(got["remap"][-1]) == exp["counter"]
    assert {i for i, s in zip(ref_ids, got["suspicious_ref"]) if s} == exp["suspicious_ref"]
    assert {i: int(s) for i, s in zip(det_ids, got["suspicious_det"]) if s} == exp["suspicious_det"]
    for k in ("label_tracked", "label_reference", "label_merged"):
        assert np.array_equal(got[k], exp[k]), k


def test_full_frame_components_and_bands_cross_tiles():
    H, W, n = 480, 640, 8
    ref, det = _label_pair(H, W, n, 3)
    ref_ids, det_ids = list(range(1, n + 1)), list(range(n))
    exp = T.track(ref, det, 20)  # the reference's own thresholds
    rows, cols = np.nonzero(exp["reference_small_removed"] == 1)
    assert cols.max() - cols.min() + 1 > 256 and rows.max() - rows.min() + 1 > 1  # one component, many workgroups
    assert (exp["reference_small_removed"] != exp["reference_relabelled"]).any()
    assert len(exp["new_ids"]) == 0 and sum(t >= 0 for t in exp["remap"].values()) >= 4
    a = _track_on_device(ref, det, ref_ids, det_ids, 20, None)
    b = _track_on_device(ref, det, ref_ids, det_ids, 20, None)
    _check_track(a, exp, ref_ids, det_ids)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k


@pytest.mark.parametrize("n", [3, 40])
def test_overlap_on_both_paths(n):
    """3 x 3 ids: the bins fit in LDS; 40 x 40: 2000 bins, the global-atomic path."""
    H, W = 121, 163
    assert (_lib.lib().mf_occtrack_stats_elems(n, n) <= 1024) == (n == 3)
    rs = np.random.RandomState(n)
    ref = (rs.randint(0, n, (H // 8 + 1, W // 8 + 1)).repeat(8, 0).repeat(8, 1)[:H, :W] + 1).astype(np.int32)
    det = rs.randint(0, n, (H // 5 + 1, W // 5 + 1)).repeat(5, 0).repeat(5, 1)[:H, :W].astype(np.int32)
    ref[rs.uniform(size=ref.shape) < 0.1] = -2
    det[rs.uniform(size=det.shape) < 0.1] = -1
    ref_ids, det_ids = list(range(1, n + 1)), list(range(n))
    th = dict(THRESHOLDS, min_area=6, band=1)
    got = _track_on_device(ref, det, ref_ids, det_ids, 100, th)
    inter, sref, sdet, box = T.overlap_stats(ref, det, ref_ids, det_ids)
    stats = got["stats"].astype(np.int64)
    assert np.array_equal(stats[:n * n].reshape(n, n), inter) and inter.sum() > 0
    assert np.array_equal(stats[n * n:n * n + 3 * n].reshape(n, 3), sref)
    assert np.array_equal(stats[n * n + 3 * n:n * n + 6 * n].reshape(n, 3), sdet)
    assert np.array_equal(stats[n * n + 6 * n:].reshape(n, 4), box)
    _check_track(got, T.track(ref, det, 100, th), ref_ids, det_ids)
    again = _track_on_device(ref, det, ref_ids, det_ids, 100, th)
    assert all(np.array_equal(v, again[k]) for k, v in got.items() if isinstance(v, np.ndarray))


@pytest.fixture(scope="module")
def sequence():
    from morefusion_amd import geometry
    frames = synthetic.make_tracking_sequence(SEED_SEQUENCE, 3, 121, 163, n_objects=5, appear_at={3: 2})
    for f in frames:
        K = f["K"]
        f["pcd"] = geometry.pointcloud_from_depth(f["depth"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    return frames


def test_three_frame_sequence_keeps_ids(sequence):
    pitch_of = C.make_pitch_of(163)
    got, m = C.run_sequence_product(sequence, THRESHOLDS, pitch_of, "cuda", as_tensor=True)
    host, mh = C.run_sequence_product(sequence, THRESHOLDS, pitch_of, "cuda", as_tensor=False)
    exp, ref = C.run_sequence_mirror(sequence, THRESHOLDS, pitch_of, [g["boxes"] for g in got])
    ids_of_object = {}
    for f, g, h, e in zip(sequence, got, host, exp):
        assert g["remap"] == e["remap"] == h["remap"] and g["counter"] == e["counter"]
        for k in ("label_tracked", "label_merged", "label_rendered"):
            assert isinstance(g[k], torch.Tensor) and isinstance(h[k], np.ndarray)
            assert np.array_equal(g[k].cpu().numpy(), e[k]) and np.array_equal(h[k], e[k]), k
        for det, tid in g["remap"].items():
            if tid >= 0:
                ids_of_object.setdefault(f["object_of_detection"][det], []).append(tid)
    stable = [o for o, t in ids_of_object.items() if len(t) == 3]
    assert len(stable) >= 3 and all(len(set(ids_of_object[o])) == 1 for o in ids_of_object)  # one id per object
    assert ids_of_object[3] == [got[2]["counter_before"]] and got[2]["counter"] == got[2]["counter_before"] + 1
    C.logodds_equal(m, ref)
    last, tracked = exp[2], exp[2]["label_tracked"]
    tids = [t for t in sorted(set(got[2]["remap"].values())) if t >= 0 and (tracked == t).any()]
    pitch = np.array([pitch_of(last["classes"][t]) for t in tids])
    pts = last["pts_map"].reshape(tracked.shape + (3,))
    origin = np.stack([np.nanmedian(pts[tracked == t], axis=0) for t in tids]).astype(np.float64) - 15.5 * pitch[:, None]
    grids = m.get_target_grids_batch(tids, torch.as_tensor(pitch).cuda(), torch.as_tensor(origin).cuda())
    for b, t in enumerate(tids):
        e = ref.get_target_grids(t, dimensions=(32, 32, 32), pitch=pitch[b], origin=origin[b])
        for g, x in zip(grids, e):
            assert np.array_equal(g[b].cpu().numpy(), x), t
        assert (e[0] > 0).any()


def test_multiview_example_end_to_end():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "multiview_mapping.py"), "--frames", "3"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    tables = re.findall(r"frame (\d+): ids \{([^}]*)\}", p.stdout)
    assert [int(k) for k, _ in tables] == [0, 1, 2]
    assert re.search(r"stable ids: (\d+) of (\d+) objects", p.stdout)
    n_stable, n_objects = map(int, re.search(r"stable ids: (\d+) of (\d+) objects", p.stdout).groups())
    assert n_stable == n_objects > 0
