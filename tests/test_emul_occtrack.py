"""csrc/occtrack.hip (with csrc/occmap.hip) through the host emulator behind the product's Python layer
(contrib.InstanceTracker, MultiInstanceOctreeMapping.integrate_tracked_frame; torch CPU tensors as device memory):
the two-frame scenario of tests/occtrack_cases.py at 48 x 64 with 3 instances -- frame 0 integrated, frame 1 from
another sensor pose with permuted detection ids -- every output bitwise equal to the mirror (tests/occtrack_ref.py),
and the maps after integrate_tracked_frame equal to tests/occmap_ref.py driven with the same tracked labels."""
import numpy as np
import pytest

import occtrack_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

THRESHOLDS = dict(min_mask=4, min_bbox=6, min_side=4, min_area=12, band=1, iou=0.4, coverage=0.9)


@pytest.fixture(scope="module")
def scenario():
    return C.make_scenario(0, 48, 64, 3, THRESHOLDS)


@pytest.fixture()
def product(monkeypatch):
    L = emul.build(["occmap.hip", "occtrack.hip"])
    emul.patch_lib(L, monkeypatch)


def test_two_frames_bitwise_vs_mirror(scenario, product):
    got, m, trk = C.run_product(scenario, "cpu")
    exp, ref = C.run_mirror(scenario, got["boxes"])
    C.check_cases(scenario, exp)  # the mirror alone shows every case the kernels branch on
    g0, e0 = got["frame0"], exp["frame0"]
    assert np.array_equal(g0["pts_map"], e0["pts_map"], equal_nan=True)
    assert (g0["label_rendered"] == -2).all()
    assert np.array_equal(g0["label_tracked"], e0["label_tracked"])
    assert np.array_equal(g0["label_merged"], e0["label_merged"]) and (g0["label_merged"] == -2).all()
    assert g0["classes"] == e0["classes"] and len(g0["classes"]) == 3
    assert np.array_equal(got["slab"], exp["slab"])
    C.check_frame1(got, exp)
    assert all(isinstance(x, np.ndarray) for x in (g0["label_tracked"], got["frame1"]["label_merged"]))
    C.logodds_equal(m, ref)
    assert int(m._overflow[0]) == 0
    for t in m._trees.values():
        assert t.bits is None or not t.bits.any()


def test_second_frame_needs_the_tracked_insert(scenario, product):
    """integrate_frame stays a one-frame builder (a second frame with the same ids raises); the tracked insert takes
    frame after frame and only initialises ids it has not seen."""
    from morefusion_amd.contrib import MultiInstanceOctreeMapping
    f0 = scenario["frames"][0]
    label = f0["label_detected"] + 1
    ids = sorted(f0["class_ids_by_detection"])
    m = MultiInstanceOctreeMapping(device="cpu")
    args = (f0["pcd"], label, [i + 1 for i in ids], [f0["class_ids_by_detection"][i] for i in ids], scenario["pitch_of"])
    m.integrate_frame(*args)
    with pytest.raises(ValueError, match="already exists"):
        m.integrate_frame(*args)
    t = MultiInstanceOctreeMapping(device="cpu")
    classes = {i + 1: f0["class_ids_by_detection"][i] for i in ids}
    tracked = np.where(label == 0, -1, label).astype(np.int32)
    for _ in range(2):
        t.integrate_tracked_frame(f0["pcd"], tracked, classes, scenario["pitch_of"])
    assert t.instance_ids == [i + 1 for i in ids] + [0]
    with pytest.raises(ValueError, match=">= 1"):
        t.integrate_tracked_frame(f0["pcd"], tracked, {0: 1}, scenario["pitch_of"])
