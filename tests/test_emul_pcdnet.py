"""csrc/pcdnet.hip (stem, pool, bias + ReLU + split) and mf_pose_epilogue as the point-cloud baseline network uses it,
through the host emulator (torch CPU tensors as device memory): B = 3, P = 37 and B = 1, P = 1, bitwise against the
NumPy mirror (tests/pcdnet_ref.py) and within the derived fp32 bound of float64; launcher refusals
(tests/pcdnet_cases.py has the checks; tests/test_gpu_pcdnet.py runs the same ones on the MI355X)."""
import pytest

import pcdnet_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture()
def dev(monkeypatch):
    emul.patch_lib(emul.build(["pcdnet.hip", "pointops.hip"]), monkeypatch)
    return "cpu"


def test_stem_bitwise_vs_mirror_and_within_fp32_bound(dev):
    C.check_stem(dev)


def test_pool_fixed_order_and_run_to_run(dev):
    C.check_pool(dev)


def test_bias_relu_split_bitwise(dev):
    C.check_bias_relu_split(dev)


def test_epilogue_reference_rounding_order(dev):
    C.check_epilogue(dev)


def test_launcher_refusals(dev):
    C.check_refusals(dev)
