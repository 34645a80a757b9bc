"""csrc/posemetric.hip through the host emulator behind the product's Python layer (metrics.average_distance_device;
torch CPU tensors as device memory), clouds of 1 .. 300 points: bitwise against the NumPy mirror
(tests/posemetric_ref.py), exact known answers, the project's host function and the reference's recorded ADD, errors
(tests/posemetric_cases.py has the checks; tests/test_gpu_posemetric.py runs the same ones on the MI355X with clouds
of up to 2620 points)."""
import pytest

import posemetric_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")
SIZES, ITEMS = C.EMUL_SIZES, 14


@pytest.fixture()
def dev(monkeypatch):
    emul.patch_lib(emul.build(["posemetric.hip"]), monkeypatch)
    return "cpu"


def test_mirror_alone_meets_host_function_and_golden():
    C.check_mirror_alone(SIZES, ITEMS)


def test_bitwise_vs_mirror_item_order_and_alone(dev):
    C.check_bitwise(dev, SIZES, ITEMS)


def test_known_answers(dev):
    C.check_known_answers(dev, 3)


def test_host_function_and_reference_golden(dev):
    C.check_host_and_golden(dev, SIZES, ITEMS)


def test_errors(dev):
    C.check_errors(dev)


def test_cpu_tensors_are_refused_without_the_emulator():
    import numpy as np
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.average_distance_device([np.zeros((4, 3))], np.eye(4)[None], np.eye(4)[None], device="cpu")
