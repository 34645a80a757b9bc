"""TEST INFRASTRUCTURE: the pose-metric checks shared by tests/test_emul_posemetric.py (host emulator, clouds of up to
300 points) and tests/test_gpu_posemetric.py (MI355X, up to 2620 points and 40 items).  Every check takes the device
and the size scale (the cloud sizes, the number of items); bounds and cases are the same on both.  The mirror is
tests/posemetric_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch

import posemetric_ref as PR
import morefusion_amd as mf
from morefusion_amd.metrics import average_distance_device

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_average_distance.npz")
EMUL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 300)  # around the wave, the tile of 256 and past it
GPU_SIZES = EMUL_SIZES + (1000, 2620)
# the host function against the kernel: its BLAS transform may order the three products of a coordinate differently,
# a few ulp of the < 2 m coordinates (< 1e-15); distance and min are 1-Lipschitz in each point, so results differ by
# < 1e-14
HOST_ATOL = 1e-12


def same_bits(got, ref, what=""):
    """float64 arrays: NaN in the same places, every other element equal bit for bit (as tests/picking_cases.py)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    diff = got[~nan].view(np.int64) != ref[~nan].view(np.int64)
    assert not diff.any(), (what, int(diff.sum()), got[~nan][diff][:4], ref[~nan][diff][:4])


def rigid(rs, near=None):
    """A random rigid transform: a uniform rotation, a translation within 1 m per axis (coordinates stay < 2 m).
    ``near``: a small motion instead, a turn of about ``near`` rad and a shift within ``near`` / 5 m."""
    q = rs.normal(size=4) if near is None else np.array([1.0, 0.0, 0.0, 0.0]) + 0.5 * near * rs.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rs.uniform(-1.0, 1.0, 3) if near is None else rs.uniform(-near / 5, near / 5, 3)
    return T


@functools.lru_cache(maxsize=None)
def scenario(sizes, n_items):
    """Clouds of the given sizes (every other one float32), ``n_items`` items that walk the clouds so that several
    share one, a true pose and a nearby predicted pose each; the mirror's answers with and without translation.
    Computed once per scale and left unchanged."""
    rs = np.random.RandomState(20 + len(sizes))
    clouds = [rs.uniform(-0.15, 0.15, (n, 3)).astype(np.float32 if m % 2 else np.float64)
              for m, n in enumerate(sizes)]
    # every size is scored, in no particular order, and the further items share those clouds
    index = np.concatenate([rs.permutation(len(sizes)), rs.randint(0, len(sizes), n_items - len(sizes))])
    T1 = np.stack([rigid(rs) for _ in range(n_items)])
    T2 = np.stack([rigid(rs) for _ in range(n_items)])
    for i in range(0, n_items, 2):  # half of the items: a small pose error, the regime of a refined pose
        T2[i] = T1[i] @ rigid(rs, near=0.05)
    ref = {tr: PR.average_distance(clouds, T1, T2, translate=tr, cloud_index=index) for tr in (True, False)}
    for v in list(ref.values()) + [T1, T2, index] + clouds:
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return clouds, index, T1, T2, ref


def run(dev, clouds, T1, T2, translate=True, index=None):
    adds, add_ss = average_distance_device(list(clouds), T1, T2, translate=translate, cloud_index=index, device=dev)
    assert adds.dtype == add_ss.dtype == torch.float64 and adds.device.type == torch.device(dev).type
    return adds.cpu().numpy(), add_ss.cpu().numpy()


def check_bitwise(dev, sizes, n_items):
    clouds, index, T1, T2, ref = scenario(sizes, n_items)
    assert len(set(index.tolist())) == len(sizes) and n_items > len(sizes)  # every size, and shared clouds
    for translate in (True, False):
        got = run(dev, clouds, T1, T2, translate, index)
        same_bits(got[0], ref[translate][0], f"add translate={translate}")
        same_bits(got[1], ref[translate][1], f"add_s translate={translate}")
    # the items permuted: the same bits after un-permuting
    perm = np.random.RandomState(3).permutation(n_items)
    again = run(dev, clouds, T1[perm], T2[perm], True, index[perm])
    inv = np.argsort(perm)
    same_bits(again[0][inv], ref[True][0], "add, permuted")
    same_bits(again[1][inv], ref[True][1], "add_s, permuted")
    # an item alone (I = 1, its cloud the only one): the same bits as inside the batch -- once per cloud size
    for c in range(len(sizes)):
        i = int(np.flatnonzero(index == c)[0])
        alone = run(dev, [clouds[c]], T1[i:i + 1], T2[i:i + 1])
        same_bits(alone[0], ref[True][0][i:i + 1], f"add alone, P={sizes[c]}")
        same_bits(alone[1], ref[True][1][i:i + 1], f"add_s alone, P={sizes[c]}")


def lattice(m):
    """(2 m + 1)^3 points on the integer lattice / 1024: symmetric under a quarter turn about z; every coordinate,
    and every sum below, is exact in float64."""
    g = np.arange(-m, m + 1, dtype=np.float64) / 1024.0
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def check_known_answers(dev, m):
    rs = np.random.RandomState(5)
    pts = lattice(m)
    assert pts.shape[0] > 256  # more than one query block, more than one target tile
    # identity pair
    T = rigid(rs)
    add, add_s = run(dev, [pts], T[None], T[None])
    assert add[0] == 0.0 and add_s[0] == 0.0
    # exact 0 / +-1 rotation and dyadic translation, the other pose 0.25 further along x: |a - b| = 0.25 for every point
    T1 = np.array([[0.0, -1.0, 0.0, 0.5], [0.0, 0.0, 1.0, -0.25], [-1.0, 0.0, 0.0, 0.75], [0.0, 0.0, 0.0, 1.0]])
    T2 = T1.copy()
    T2[0, 3] += 0.25
    add, add_s = run(dev, [pts], T1[None], T2[None])
    assert add[0] == 0.25 and 0.0 < add_s[0] <= 0.25
    # a quarter turn about z maps the lattice onto itself: every point has a neighbour at distance 0
    Rz = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    T1 = np.eye(4)
    T1[:3, 3] = (0.5, -0.25, 0.75)
    add, add_s = run(dev, [pts], T1[None], (T1 @ Rz)[None])
    assert add_s[0] == 0.0 and add[0] > 0.0
    # translate=False: poses that differ in translation only are the same pose
    T1 = rigid(rs)
    T2 = T1.copy()
    T2[:3, 3] = rs.uniform(-1.0, 1.0, 3)
    add, add_s = run(dev, [pts], T1[None], T2[None], translate=False)
    assert add[0] == 0.0 and add_s[0] == 0.0
    add, add_s = run(dev, [pts], T1[None], T2[None], translate=True)
    assert add[0] > 0.0


def host_and_golden(score):
    """``score(clouds, T1, T2, translate, index) -> (adds, add_ss)`` against metrics.average_distance and the
    reference's recorded ADD (the check of tests/test_host_logic.py, at its rtol)."""
    def check(clouds, index, T1, T2):
        for translate in (True, False):
            add, add_s = score(clouds, T1, T2, translate, index)
            h_add, h_add_s = mf.metrics.average_distance([np.asarray(clouds[c]) for c in index], list(T1), list(T2),
                                                         translate=translate)
            print(f"translate={translate}: max |add - host| = {np.abs(add - h_add).max():.3e}, "
                  f"max |add_s - host| = {np.abs(add_s - h_add_s).max():.3e}")
            np.testing.assert_allclose(add, h_add, rtol=0, atol=HOST_ATOL)
            np.testing.assert_allclose(add_s, h_add_s, rtol=0, atol=HOST_ATOL)
            assert (add_s <= add).all()
    return check


def check_host_and_golden(dev, sizes, n_items, score=None):
    clouds, index, T1, T2, _ = scenario(sizes, n_items)
    if score is None:
        def score(clouds, T1, T2, translate, index):
            return run(dev, clouds, T1, T2, translate, index)
    host_and_golden(score)(clouds, index, T1, T2)
    g = np.load(GOLDEN)
    n = g["transforms_pred"].shape[0]
    add, add_s = score([g["points"]], np.stack([g["transform_true"]] * n), g["transforms_pred"], True,
                       np.zeros(n, np.int64))
    np.testing.assert_allclose(add, g["add"], rtol=1e-5)
    assert (add_s <= add).all()


def check_mirror_alone(sizes, n_items):
    """Before any kernel runs: the mirror itself meets the host function's and the golden's bounds."""
    def score(clouds, T1, T2, translate, index):
        return PR.average_distance(clouds, T1, T2, translate=translate, cloud_index=index)
    check_host_and_golden(None, sizes, n_items, score)


def check_errors(dev):
    rs = np.random.RandomState(1)
    pts = rs.uniform(-0.1, 0.1, (5, 3))
    T = np.stack([rigid(rs), rigid(rs)])
    with pytest.raises(ValueError):  # an empty cloud
        average_distance_device([pts, np.zeros((0, 3))], T, T, device=dev)
    with pytest.raises(ValueError):  # lengths
        average_distance_device([pts], T, T, device=dev)
    with pytest.raises(ValueError):
        average_distance_device([pts, pts], T, T[:1], device=dev)
    with pytest.raises(ValueError):  # transforms that are not 4 x 4
        average_distance_device([pts, pts], T[:, :3], T, device=dev)
    with pytest.raises(ValueError):  # points that are not [n, 3]
        average_distance_device([pts[:, :2], pts], T, T, device=dev)
    for bad in ([0, 1], [-1, 0], [0]):  # a cloud index out of range; an index list of another length
        with pytest.raises(ValueError):
            average_distance_device([pts], T, T, cloud_index=bad, device=dev)
    add, add_s = average_distance_device([pts], T, T, cloud_index=[0, 0], device=dev)  # ... and a good one
    assert add.cpu().tolist() == [0.0, 0.0] and add_s.cpu().tolist() == [0.0, 0.0]
    add, add_s = average_distance_device([], np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), device=dev)  # no items
    assert add.shape == add_s.shape == (0,)
