"""csrc/pickorder.hip on the MI355X at 480 x 640: the checks of tests/test_emul_picking.py (tests/picking_cases.py)
-- bitwise against the NumPy mirror and the reference's recorded normals, known answers, edge cases."""
import pytest

import picking_cases as C

pytestmark = pytest.mark.gpu
H, W = 480, 640
DEV = "cuda"


def test_bitwise_vs_mirror_and_item_order():
    C.check_bitwise(DEV, H, W)


def test_normals_vs_mirror_reference_and_crop():
    C.check_normals(DEV, H, W)


def test_plane_normals():
    C.check_plane_normals(DEV, H, W)


def test_known_answers():
    C.check_known_answers(DEV, H, W)


def test_edge_cases():
    C.check_edges(DEV, H, W)


def test_max_objects():
    C.check_max_objects(DEV)
