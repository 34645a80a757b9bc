"""csrc/posemetric.hip on the MI355X: the checks of tests/test_emul_posemetric.py (tests/posemetric_cases.py) with
clouds of up to 2620 points (a dense YCB model cloud) and 40 items -- bitwise against the NumPy mirror, exact known
answers, the project's host function and the reference's recorded ADD, errors."""
import pytest

import posemetric_cases as C

pytestmark = pytest.mark.gpu
SIZES, ITEMS = C.GPU_SIZES, 40
DEV = "cuda"


def test_bitwise_vs_mirror_item_order_and_alone():
    C.check_bitwise(DEV, SIZES, ITEMS)


def test_known_answers():
    C.check_known_answers(DEV, 6)


def test_host_function_and_reference_golden():
    C.check_host_and_golden(DEV, SIZES, ITEMS)


def test_errors():
    C.check_errors(DEV)
