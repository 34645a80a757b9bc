"""conv3's 16 occupancy channels as a split-bf16 GEMM on the MI355X (the precision contract is 8.1's):

* mf_conv3d_k4s2_split_fwd at Cin 16 / Cout 256 / D 8 on every tile form, 1 and 2 objects: |y - y_fp64| <= 2^-15
  conv(|x|, |w|)_fp64 per element, two runs bitwise equal, and a single voxel through a single tap lands where the
  arithmetic by hand puts it;
* the second occupancy convolution's split store is ``mf_split_bf16`` of the fp32 grid the parent path writes;
* ``Model.predict`` at 4 objects with the layer's switch on against off within 2e-4; one object launches none of it."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import morefusion_amd as mf  # noqa: E402
from morefusion_amd import _lib  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import Model, volumetric_cl  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models.volumetric_cl import ChannelsLastVolumetric  # noqa: E402
import volumetric_split2_ref as R  # noqa: E402

KEYS = ("class_id", "rgb", "pcd", "pitch", "origin", "grid_nontarget_empty")


@pytest.fixture(params=list(R.FORMS))
def form(request, monkeypatch):
    for k in ("MF_NT_BIG", "MF_NT_SPLITK", "MF_NT_HALF_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in R.FORMS[request.param][0].items():
        monkeypatch.setenv(k, v)
    return request.param


def test_occupancy_split_store():
    R.check_occupancy_split_store(_lib.lib(), "cuda", _lib.stream_ptr())


@pytest.mark.parametrize("B", [1, 2])
def test_conv3_occ_error_bound(form, B):
    R.check_conv3_occ_bound(_lib.lib(), "cuda", _lib.stream_ptr(), form, B)


def test_conv3_occ_single_voxel_single_tap(form):
    R.check_single_voxel_single_tap(_lib.lib(), "cuda", _lib.stream_ptr(), form)


def _inputs(B, seed=7):
    b = mf.synthetic.make_singleview_batch(B, seed=seed)
    return b, {k: torch.as_tensor(b[k]).cuda() for k in KEYS}


def _predict(model, inputs, on):
    saved = ChannelsLastVolumetric.split_conv3_occ
    ChannelsLastVolumetric.split_conv3_occ = on
    try:
        with torch.no_grad():
            model.predict(**inputs)
            return tuple(x.cpu() for x in model.predict(**inputs))
    finally:
        ChannelsLastVolumetric.split_conv3_occ = saved


def _record(monkeypatch):
    calls = []
    for name in ("conv_k4s2", "conv_k4s2_split"):
        f = getattr(ChannelsLastVolumetric, name)
        monkeypatch.setattr(ChannelsLastVolumetric, name,
                            lambda self, layer, *a, _f=f, _n=name, **k: (calls.append((_n, layer)), _f(self, layer, *a, **k))[1])
    return calls


def test_predict_on_vs_off_at_four_objects(monkeypatch):
    torch.backends.cudnn.benchmark = False
    torch.manual_seed(0)
    B = 4
    assert volumetric_cl.SPLIT_MIN_BATCH["conv3_occ"] <= B
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    b, inputs = _inputs(B)
    calls = _record(monkeypatch)
    on = _predict(model, inputs, True)
    assert ("conv_k4s2_split", "conv3_occ") in calls and ("conv_k4s2", "conv3_occ") not in calls
    del calls[:]
    off = _predict(model, inputs, False)
    assert ("conv_k4s2", "conv3_occ") in calls and ("conv_k4s2_split", "conv3_occ") not in calls
    pitch = np.asarray(b["pitch"], np.float32).reshape(B, 1, 1)
    (rot_s, trans_s, conf_s), (rot_m, trans_m, conf_m) = on, off
    print("predict B=4 conv3_occ on vs off: rot %.3g conf %.3g trans/pitch %.3g" % (
        float((rot_s - rot_m).abs().max()), float((conf_s - conf_m).abs().max()),
        float(np.abs(trans_s.numpy() / pitch - trans_m.numpy() / pitch).max())))
    np.testing.assert_allclose(rot_s.numpy(), rot_m.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(conf_s.numpy(), conf_m.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(trans_s.numpy() / pitch, trans_m.numpy() / pitch, rtol=0, atol=2e-4)


def test_one_object_launches_none_of_it(monkeypatch):
    """Below the table the volumetric part launches the parent's kernels: no call of the split operators, and the NT
    engine's last-tile record still shows the 128-row launch made right before it (the layer at one object would have
    taken the 256-row tile: 16 tiles, split-K 3)."""
    L = _lib.lib()
    t, s = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.mf_gemm_bf16_nt_plan(R.MODE_CONV3_SPLIT, 16 ** 3, R.COUT, 64 * 3 * R.CIN, 1, 0, 0, 1, 1, ctypes.byref(t),
                                  ctypes.byref(s)) == 0 and t.value == 256
    torch.manual_seed(0)
    model = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    vol = ChannelsLastVolumetric(model)
    assert ChannelsLastVolumetric.split_bf16 and ChannelsLastVolumetric.split_conv3_occ
    _, inp = _inputs(1)
    with torch.no_grad():
        assert not vol._split_path("conv3_occ", 1) and vol._split_path("conv3_occ", 4)
        pix = model._select_points(inp["pcd"])
        values, points = model._backbone_features(inp["rgb"], inp["pcd"], pix)
    x, W = R.conv3_occ_problem(1)
    with monkeypatch.context() as mp:   # a fresh 128-row launch of the engine
        for k, v in R.FORMS["tile128"][0].items():
            mp.setenv(k, v)
        R.run_conv3_occ(L, "cuda", _lib.stream_ptr(), x, R.pack(L, W, "cuda", _lib.stream_ptr()), 128, False)
    calls = _record(monkeypatch)
    with torch.no_grad():
        feat, _ = vol.features(values, points, inp["pitch"].float(), inp["origin"].float(), inp["grid_nontarget_empty"],
                               occ_split=True)
        torch.cuda.synchronize()
    assert L.mf_gemm_bf16_last_tile() == 128
    assert calls == [("conv_k4s2", "conv3_occ"), ("conv_k4s2", "conv4")], calls
    assert getattr(feat, "_mf_split", None) is None
