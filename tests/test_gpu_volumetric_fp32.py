"""The fp32 3-D inference kernels on the MI355X: the cases of tests/volumetric_fp32_cases.py (its docstring says which
case reaches which branch of csrc/linear.hip, conv3d.hip, sparseconv.hip, interp.hip, pointops.hip) through the C ABI,
against the float64 references, the bit-exact mirrors and the a-priori bound |got - ref| <= 2 K 2^-24 S of
tests/volumetric_fp32_ref.py -- the same checks as tests/test_emul_volumetric_fp32.py, here with the real MFMA lane
layouts, barriers, workgroup remap, atomics and wave intrinsics -- and one small chain through
``ChannelsLastVolumetric.features`` / ``heads`` checked stage by stage.

Worst |got - ref| / bound per kernel, MEASURED ON ONE RUN on the MI355X (the bound is derived; these only show its slack):
    mf_linear_fwd                            0.063   (chain: 0.244, conv1_pcd at K = 4)
    mf_conv3d_k4s2_fwd, split 1              0.002   (chain: 0.001)
    mf_conv3d_k4s2_fwd + k_conv_finish       0.004
    mf_occupancy_convs_fwd h1 / h2           0.034 / 0.007   (chain: 0.048 / 0.011)
    sparse conv3 fp32 (all entries)          0.004   (chain: below 0.0005)
    mf_pose_epilogue                         0.551   (of losschain_ref's bound, which ASSUMES 2 ulp for sqrtf / expf / divide)
    mf_to_channels_last, mf_interpolate_voxel_grid_cl_fwd, mf_point_prep, the two packs: equal bits
"""
import numpy as np
import pytest
import torch

import volumetric_fp32_cases as C
import volumetric_fp32_ref as R

pytestmark = pytest.mark.gpu

from morefusion_amd import _lib  # noqa: E402


class Dev:
    """torch CUDA tensors as device memory: the twin of volumetric_fp32_cases.Host."""
    @staticmethod
    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    @staticmethod
    def host(t):
        return t.cpu().numpy()

    @staticmethod
    def ptr(t, off=0):
        return None if t is None else t.data_ptr() + off * t.element_size()

    @property
    def stream(self):
        return _lib.stream_ptr()

    @staticmethod
    def sync():
        torch.cuda.synchronize()


X = Dev()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    C.report()


@pytest.mark.parametrize("name", list(C.LINEAR))
def test_linear_every_element_within_its_bound(name):
    C.check_linear(name, C.run_linear(_lib.lib(), X, name), "gpu")


def test_linear_refusals():
    C.check_linear_refusals(_lib.lib(), X)


@pytest.mark.parametrize("name", list(C.CONV))
def test_conv3d_k4s2_every_element_within_its_bound(name):
    got = C.run_conv(_lib.lib(), X, name)
    C.check_conv(name, got, "gpu")
    if C.CONV[name]["split"] == "max":
        C.bits_equal(C.run_conv(_lib.lib(), X, name)["out"], got["out"], f"conv {name}: a second launch")


def test_conv3d_refusals():
    C.check_conv_refusals(_lib.lib(), X)


@pytest.mark.parametrize("name", list(C.OCC))
def test_occupancy_convs_every_element_within_its_bound(name):
    C.check_occ(name, C.run_occ(_lib.lib(), X, name), "gpu")


@pytest.mark.parametrize("shape", C.TCL)
def test_to_channels_last_bits(shape):
    C.run_check_tcl(_lib.lib(), X, shape, "gpu")


@pytest.mark.parametrize("name", list(C.SPARSE))
def test_sparse_conv3_every_entry_within_its_bound_and_bit_equal(name):
    C.check_sparse(_lib.lib(), X, name, "gpu")


@pytest.mark.parametrize("shape", C.INTERP)
def test_interpolate_channels_last_bits(shape):
    C.run_check_interp(_lib.lib(), X, shape, "gpu")


@pytest.mark.parametrize("shape", C.PREP)
def test_point_prep_bits_and_pose_epilogue_within_its_bound(shape):
    C.run_check_prep(_lib.lib(), X, shape, "gpu")


def test_chain_stage_by_stage():
    """(B, P) = (2, 37), D = 32 through ``ChannelsLastVolumetric.features`` and ``heads`` with ``split_bf16 = False``:
    every stage is checked on the fp32 tensors the device itself handed to it (the stage methods are called again on
    those tensors where ``features`` does not return an intermediate; what ``features`` assembled must then be the same
    bits).  This also checks that the Python layer passes the strides and column offsets the kernels were tested with."""
    from morefusion_amd.contrib.singleview_3d.models import Model
    from morefusion_amd.contrib.singleview_3d.models.volumetric_cl import F_COLS, F_LD, ChannelsLastVolumetric
    torch.manual_seed(3)
    m = Model(n_fg_class=21, with_occupancy=True).cuda().eval()
    vol = ChannelsLastVolumetric(m)
    vol.split_bf16 = False
    B, P, D, nf = 2, 37, 32, 21
    n = B * P
    rs = np.random.RandomState(17)
    pitch = rs.uniform(0.004, 0.01, B).astype(np.float32)
    origin = rs.uniform(-0.4, 0.2, (B, 3)).astype(np.float32)
    pc = (origin[:, :, None] + pitch[:, None, None] * rs.uniform(-0.4, 31.4, (B, 3, P))).astype(np.float32)
    vals = rs.uniform(-1, 1, (B, 32, P)).astype(np.float32)
    grid = (rs.uniform(size=(B, D, D, D)) < 0.3).astype(np.float32)
    h = lambda t: t.detach().cpu().numpy()  # noqa: E731
    op = "gpu chain"
    with torch.no_grad():
        args = [X.dev(a) for a in (vals, pc, pitch, origin)]
        feat, pts = vol.features(*args, X.dev(grid))
        pts_k, tc4, x_rgb, bi = vol.prep(*args)
        f = h(feat)
        assert feat.shape == (n, F_LD) and (f[:, F_COLS:] == 0).all()
        # mf_point_prep: bits
        want = R.point_prep(pc, vals, origin, pitch, D / 2.0 - 0.5)
        for got, w, k in zip((pts_k, tc4, x_rgb, bi), want, ("pts", "tc4", "rows", "batch indices")):
            C.bits_equal(h(got), w, "chain point_prep " + k)
        C.bits_equal(h(pts), want[0], "chain features' points")
        # the point MLP: each layer on the columns the device handed to it

        def lin(conv, a, out, what, k_pad=None):
            w = h(conv.weight).squeeze(-1)
            ref, S, K = R.linear(a[:, :w.shape[1]], w, h(conv.bias), True)
            R.assert_within(out, ref, S, K, "chain " + what, op=op + " mf_linear_fwd")
        lin(m.conv1_rgb, want[2], f[:, 0:64], "conv1_rgb")
        lin(m.conv1_pcd, want[1], f[:, 64:72], "conv1_pcd")
        lin(m.conv2_rgb, f[:, 0:64], f[:, 72:200], "conv2_rgb")
        lin(m.conv2_pcd, f[:, 64:72], f[:, 200:216], "conv2_pcd")
        # occupancy branch and conv3's occupancy channels
        h_occ = vol.occupancy(X.dev(grid))
        h1 = h(vol._scratch("occ_h1", (B, D ** 3, 8), h_occ.device))
        C.check_occ_values(grid, h(m.conv1_occ.weight), h(m.conv1_occ.bias), h(m.conv2_occ.weight), h(m.conv2_occ.bias),
                           h1, h(h_occ), "chain occupancy", op + " mf_occupancy_convs_fwd")
        dense = vol.conv_k4s2("conv3_occ", m.conv3, h_occ, B, D, cin=16, c_off=144, relu=False, bias=False)
        split = int(_lib.lib().mf_conv3d_k4s2_default_split(B, 16, 256, D))
        w3 = h(m.conv3.weight)
        ref, S = R.conv3d(C.cf(h(h_occ), D), w3[:, 144:], stride=2, pad=1)
        R.assert_within(C.cf(h(dense), D // 2), ref, S, R.conv_k4s2_K(16, split, None, None), "chain conv3 occupancy channels",
                        op=op + " mf_conv3d_k4s2_fwd")
        # sparse conv3 on the device's own feat2 columns, points and dense addend
        h3 = vol._sparse.from_points_cl(feat[:, 72:216], F_LD, pts, bi, B, dense, D)
        g3, _ = R.voxelize(np.ascontiguousarray(f[:, 72:216]), want[0], want[3], B, D)
        ref, S, K = R.sparse_conv3(g3, w3[:, :144], C.cf(h(dense), D // 2), h(m.conv3.bias), True)
        R.assert_within(C.cf(h(h3), D // 2), ref, S, K, "chain sparse conv3", op=op + " sparse conv3 fp32")
        # conv4 on the device's h3
        h4 = vol.conv_k4s2("conv4", m.conv4, h3, B, D // 2, cin=256)
        split = int(_lib.lib().mf_conv3d_k4s2_default_split(B, 256, 512, D // 2))
        ref, S = R.conv3d(C.cf(h(h3), D // 2), h(m.conv4.weight), h(m.conv4.bias), None, True, stride=2, pad=1)
        R.assert_within(C.cf(h(h4), D // 4), ref, S, R.conv_k4s2_K(256, split, True, None), "chain conv4",
                        op=op + " mf_conv3d_k4s2_fwd")
        # the samplers' column blocks of F: the mirror's bits on the device's own grids (so features' h3 / h4 are these)
        p2 = (want[0] * np.float32(0.5)).astype(np.float32)
        C.bits_equal(f[:, 216:472], R.interpolate_cl(h(h3), D // 2, p2, want[3]), "chain samples of h3")
        C.bits_equal(f[:, 472:984], R.interpolate_cl(h(h4), D // 4, (p2 * np.float32(0.5)).astype(np.float32), want[3]),
                     "chain samples of h4")
        # the heads
        o, np4 = vol.heads(feat, B, P, raw=True)
        o = h(o)
        a1, a2, a3 = (h(vol._scratch(k, (n, c), feat.device)) for k, c in (("heads_h1", 1920), ("heads_h2", 768), ("heads_h3", 384)))
        for g, k in enumerate(("rot", "trans", "conf")):
            lin(getattr(m, f"conv1_{k}"), f, a1[:, 640 * g:640 * g + 640], f"heads layer 1 {k}")
            lin(getattr(m, f"conv2_{k}"), a1[:, 640 * g:640 * g + 640], a2[:, 256 * g:256 * g + 256], f"heads layer 2 {k}")
            lin(getattr(m, f"conv3_{k}"), a2[:, 256 * g:256 * g + 256], a3[:, 128 * g:128 * g + 128], f"heads layer 3 {k}")
            c4 = getattr(m, f"conv4_{k}")
            w = h(c4.weight).squeeze(-1)
            ref, S, K = R.linear(a3[:, 128 * g:128 * g + 128], w, h(c4.bias), False)
            R.assert_within(o[:, np4 * g:np4 * g + w.shape[0]], ref, S, K, f"chain heads layer 4 {k}", op=op + " mf_linear_fwd")
            assert (o[:, np4 * g + w.shape[0]:np4 * (g + 1)] == 0).all()   # zero weight rows and biases up to np4
