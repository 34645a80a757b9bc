"""csrc/pickorder.hip (with render.hip) through the host emulator behind the product's Python layer
(contrib/picking_order.py, geometry/estimate_pointcloud_normals.py; torch CPU tensors as device memory), at 96 x 128:
bitwise against the NumPy mirror (tests/picking_ref.py) and the reference's recorded normals, known answers and edge
cases (tests/picking_cases.py has the checks; tests/test_gpu_picking.py runs the same ones on the MI355X at
480 x 640)."""
import pytest

import picking_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")
H, W = 96, 128


@pytest.fixture()
def dev(monkeypatch):
    emul.patch_lib(emul.build(["render.hip", "meshsdf.hip", "pickorder.hip"]), monkeypatch)
    return "cpu"


def test_bitwise_vs_mirror_and_item_order(dev):
    C.check_bitwise(dev, H, W)


def test_normals_vs_mirror_reference_and_crop(dev):
    C.check_normals(dev, H, W)


def test_plane_normals(dev):
    C.check_plane_normals(dev, H, W)


def test_known_answers(dev):
    C.check_known_answers(dev, H, W)


def test_edge_cases(dev):
    C.check_edges(dev, H, W)


def test_max_objects(dev):
    C.check_max_objects(dev)
