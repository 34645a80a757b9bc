"""csrc/augment.hip through the host emulator behind datasets/augmentation.py (torch CPU tensors as device memory)
at 64 x 64: bitwise against the NumPy mirror (tests/augment_ref.py), against scipy and colorsys, and the statistical
checks (tests/augment_cases.py has them; tests/test_gpu_augment.py runs the same ones on the MI355X at 256 x 256,
n = 16, where the kernel's opt-in to more than 64 KB of LDS is exercised)."""
import pytest

import augment_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")
S, N = 64, 6


@pytest.fixture()
def dev(monkeypatch):
    emul.patch_lib(emul.build(["render.hip", "meshsdf.hip", "preprocess.hip", "augment.hip"]), monkeypatch)
    return "cpu"


def test_bitwise_vs_mirror(dev):
    """Noised coordinates: bound 2^-21 m (one float32 spacing below 4 m); observed 0 here (same libm as NumPy)."""
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
    C.check_point_statistics(dev, S, 16)


def test_reference_shaped_properties(dev):
    C.check_reference_properties(dev, S, N)
