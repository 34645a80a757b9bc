"""csrc/augment.hip on the MI355X at 256 x 256, n = 16 (the mask kernel's 137 KB of LDS): the checks of
tests/augment_cases.py -- bitwise against the NumPy mirror, scipy / colorsys, statistics."""
import pytest
import torch

import augment_cases as C

pytestmark = pytest.mark.gpu
S, N = 256, 16


@pytest.fixture()
def dev():
    assert torch.cuda.is_available()
    return "cuda"


def test_bitwise_vs_mirror(dev):
    """Noised coordinates: bound 2^-21 m (one float32 spacing below 4 m)."""
    C.check_bitwise(dev, S, N)


def test_determinism_and_batch_independence(dev):
    C.check_determinism_and_batch_independence(dev, S, N)


def test_components_vs_scipy(dev):
    C.check_components(dev, S, N)


def test_blob_count_distribution(dev):
    C.check_blob_count_distribution(dev, S)


def test_hsv_round_trip_bound(dev):
    C.check_hsv_round_trip(dev, S, N)


def test_blur_vs_scipy(dev):
    C.check_blur(dev, S, N)


def test_point_statistics(dev):
    C.check_point_statistics(dev, S, N)


def test_reference_shaped_properties(dev):
    C.check_reference_properties(dev, S, N)


def test_graph_capture(dev):
    """The three stages capture into one graph (no allocation, no synchronisation inside) and replay to the same
    result."""
    import numpy as np
    from morefusion_amd.datasets import augmentation as A
    rgb, pcd = C.crops(dev, S, 4)
    rgb, pcd = torch.from_numpy(rgb).cuda(), torch.from_numpy(pcd).cuda()
    prm = A._table(A.draw_params(4, np.random.RandomState(0)), 4, rgb.device)
    ws = A._workspace(4, S, rgb.device)

    def run():
        m = A.augment_mask(rgb, pcd, prm, 9, workspace=ws)
        return A.augment_rgb(m["rgb"], prm, workspace=ws), A.augment_pcd(m["pcd"], prm, 9)
    want = [x.clone() for x in run()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(torch.nan_to_num(got[1]), torch.nan_to_num(want[1]))
