"""csrc/render.hip on the MI355X at 480 x 640: the checks of tests/test_emul_render.py (tests/render_cases.py) --
bitwise against the NumPy mirror, analytic box / icosphere, render_cad, the full grids -- and get_example on a
frame rendered from the committed YCB meshes, through transform_example into one Model loss."""
import numpy as np
import pytest
import torch

import render_cases as C
import morefusion_amd as mf

pytestmark = pytest.mark.gpu
H, W = 480, 640
DEV = "cuda"


def test_bitwise_vs_mirror_and_order_independence():
    C.check_bitwise(DEV, H, W)


def test_clipped_near_degenerate_empty():
    C.check_edge_cases(DEV, H, W)


def test_box_against_ray_box_intersection():
    C.check_box_analytic(DEV, H, W)


def test_icosphere_against_sphere():
    C.check_icosphere_analytic(DEV, H, W)


def test_render_cad():
    C.check_render_cad(DEV, H, W)


def test_full_grids():
    C.check_full_grids(DEV)


def test_get_example_schema_skips_and_loss():
    from morefusion_amd.chainer_compat import cuda, dataset
    from morefusion_amd.contrib.singleview_3d.models import Model
    ds, examples, frame, share = C.check_examples(DEV, H, W)
    C.check_skips(DEV, H, W)
    batch = dataset.concat_examples([mf.synthetic.transform_example(e) for e in examples])
    assert batch["grid_nontarget_empty"].dtype == bool and batch["grid_nontarget_empty"].any()
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(n_fg_class=21, with_occupancy=True, models=ds._models).cuda().eval()
    keys = ("class_id", "rgb", "pcd", "quaternion_true", "translation_true", "pitch", "origin", "grid_nontarget_empty")
    with torch.no_grad():
        loss = model(**{k: cuda.to_gpu(batch[k]) for k in keys})
    assert np.isfinite(float(loss))
