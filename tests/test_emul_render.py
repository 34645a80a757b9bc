"""csrc/render.hip through the host emulator behind the product's Python layer (geometry/render.py,
extra.render_cad; torch CPU tensors as device memory), at 96 x 128: bitwise against the NumPy mirror
(tests/render_ref.py), against analytic geometry, render_cad and the full grids (tests/render_cases.py has the
checks; tests/test_gpu_render.py runs the same ones on the MI355X at 480 x 640)."""
import ctypes
import re

import pytest

import render_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")
H, W = 96, 128


@pytest.fixture()
def dev(monkeypatch):
    emul.patch_lib(emul.build(["render.hip", "meshsdf.hip"]), monkeypatch)
    return "cpu"


def test_bitwise_vs_mirror_and_order_independence(dev):
    C.check_bitwise(dev, H, W)


def test_clipped_near_degenerate_empty(dev):
    C.check_edge_cases(dev, H, W)


def test_box_against_ray_box_intersection(dev):
    C.check_box_analytic(dev, H, W)


def test_icosphere_against_sphere(dev):
    C.check_icosphere_analytic(dev, H, W)


def test_render_cad(dev):
    C.check_render_cad(dev, H, W)


def test_full_grids(dev):
    C.check_full_grids(dev)


def test_render_batch_struct_matches_header():
    """mfRenderBatch is bound by reference as a plain pointer: its layout is checked here, field by field."""
    from morefusion_amd import _lib
    import os
    text = open(os.path.join(emul.ROOT, "include", "mfhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} mfRenderBatch;", text).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    kinds = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    want = [(d.split()[-1].lstrip("*"), ctypes.c_void_p if "*" in d else kinds[d.split()[0]]) for d in decls]
    assert want == list(_lib.RenderBatch._fields_)
    assert ctypes.sizeof(_lib.RenderBatch) == 14 * 8 + 5 * 8 + 6 * 4
