"""The training loss chain on the MI355X: the cases of tests/losschain_cases.py (its docstring says which case reaches
which branch of csrc/loss.hip / csrc/pointops.hip) against the float64 references and a-priori bounds of
tests/losschain_ref.py -- the same checks as tests/test_emul_losschain.py.  Values and gradients go through the Python
wrappers (``average_distance_batch``, ``confidence_loss``, ``K.PoseEpilogue``, ``transformation_matrix_batch``) and
autograd; ``_lib.lib()`` is used where only the C ABI reaches the branch (the arg-min rows, nn_idx = NULL, the
refusals, sentinel-filled outputs), and both routes must give the same bits.  The arg-min rows are bit-equal to the
float32 mirror (oracle_np.nn), which no emulator is involved in.  The ulp figures of the device's expf / logf / sqrtf
and divide behind the bounds are ASSUMED (2 ulp), not measured."""
import numpy as np
import pytest
import torch

import losschain_cases as C

pytestmark = pytest.mark.gpu

from morefusion_amd import _lib  # noqa: E402
from morefusion_amd.contrib.singleview_3d.models import bf16_ops as K  # noqa: E402
from morefusion_amd.functions.geometry.transformation_matrix import transformation_matrix_batch  # noqa: E402
from morefusion_amd.functions.loss.average_distance import average_distance_batch  # noqa: E402
from morefusion_amd.functions.loss.confidence_loss import confidence_loss  # noqa: E402


class Dev:
    """torch CUDA tensors as device memory: the twin of losschain_cases.Host."""
    @staticmethod
    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    @staticmethod
    def host(t):
        return t.cpu().numpy()

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

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


def bits(a):
    return np.asarray(a).view(np.int32)


def leaf(a):
    return X.dev(a).requires_grad_(True)


@pytest.mark.parametrize("M", C.ADD_MS)
def test_add_adds_every_element_within_its_bound(M):
    """loss_walk forward and backward: M < 4, M = 1, the staged tile (M <= 1024), the unstaged multi-tile search
    (M = 1025: a last tile of one point padded with +inf; 2051), ragged rounds, ties between tiles and inside a group of
    four, the n > 0 guard (pose [0, 0]) and grp == -1 (the NaN pose [2, 1])."""
    c = C.add_case(M)
    got = C.run_add(_lib.lib(), X, c)            # C ABI: the arg-min rows, sentinel-filled outputs
    C.check_add(c, got, "gpu")
    assert (got["idx"][0] == C.ISENT).all()
    Tp = leaf(c["T_pred"])
    out = average_distance_batch(X.dev(c["points"]), X.dev(c["T_true"]), Tp, X.dev(c["sym"]).bool())
    out.backward(X.dev(c["gout"]))
    np.testing.assert_array_equal(bits(X.host(out.detach())), bits(got["out"]))
    np.testing.assert_array_equal(bits(X.host(Tp.grad)), bits(got["gT"]))


@pytest.mark.parametrize("M", [300, 1025, 2051])
def test_add_backward_that_repeats_the_search_gives_the_same_bits(M):
    """nn_idx = NULL in the backward (C ABI only): within one tile (300) and across tiles, restaged every round (1025,
    2051)."""
    c = C.add_case(M)
    a = C.run_add(_lib.lib(), X, c, bwd_idx=True)
    b = C.run_add(_lib.lib(), X, c, bwd_idx=False, fwd_idx=False)
    np.testing.assert_array_equal(bits(a["gT"]), bits(b["gT"]))
    np.testing.assert_array_equal(bits(a["out"]), bits(b["out"]))
    if M == 300:
        C.check_add(c, a, "gpu")


@pytest.mark.parametrize("B,P", C.CONF_SHAPES)
def test_confidence_loss_every_element_within_its_bound(B, P):
    """k_conf_loss_fwd / _bwd: P < 64, a wave's second object, a lane's second round, conf == 0 exactly, and at (40, 65)
    object 23 (wave 7, second pass) without a confident point."""
    for c in [C.conf_case(B, P)] + ([C.conf_case(B, P, finite=True)] if (B, P) == (40, 65) else []):
        got = C.run_conf(_lib.lib(), X, c)
        C.check_conf(c, got, "gpu")
        add, conf = leaf(c["add"]), leaf(c["conf"])
        loss = confidence_loss(add, conf, c["lam"])
        loss.backward(X.dev(c["gloss"]).reshape(()))
        np.testing.assert_array_equal(bits(X.host(loss.detach()).reshape(1)), bits(got["loss"]))
        np.testing.assert_array_equal(bits(X.host(add.grad)), bits(got["dadd"]))
        np.testing.assert_array_equal(bits(X.host(conf.grad)), bits(got["dconf"]))
    if (B, P) == (40, 65):
        first = C.run_conf(_lib.lib(), X, C.conf_case(B, P))
        assert first["cnt"][23] == 0 and np.isnan(first["loss"][0])


def test_confidence_loss_refuses_b_0_and_b_8193():
    """Host-side argument checks (csrc/loss.hip: mf_confidence_loss_fwd returns before the launch)."""
    C.check_conf_refusals(_lib.lib(), X)


@pytest.mark.parametrize("B,P,nf", C.EPI_SHAPES)
def test_pose_epilogue_every_element_within_its_bound(B, P, nf):
    """k_pose_epi3_fwd / _bwd: n_fg = 1, B P 8 n_fg not a multiple of 256, first and last class, ids 0 and n_fg + 1
    (zero rows written over a sentinel), s == 0 and a row of norm 1e-6."""
    c = C.epi_case(B, P, nf)
    got = C.run_epi(_lib.lib(), X, c)
    C.check_epi(c, got, "gpu")
    orot, otrn, ocnf = leaf(c["orot"]), leaf(c["otrn"]), leaf(c["ocnf"])
    rot, trans, conf = K.PoseEpilogue.apply(orot, otrn, ocnf, X.dev(c["class_id"]), X.dev(c["pts"]), X.dev(c["pitch"]),
                                            X.dev(c["origin"]), B, P, nf)
    torch.autograd.backward([rot, trans, conf], [X.dev(c["grot"]), X.dev(c["gtrans"]), X.dev(c["gconf"])])
    for k, t in (("rot", rot), ("trans", trans), ("conf", conf), ("drot", orot.grad), ("dtrn", otrn.grad), ("dcnf", ocnf.grad)):
        np.testing.assert_array_equal(bits(X.host(t.detach())), bits(got[k]))


@pytest.mark.parametrize("n", C.TFM_NS)
def test_transformation_matrix_every_element_within_its_bound(n):
    """k_tfm_fwd / _bwd around a block boundary, quaternion norms 1e-3 .. 1e3; the cotangent's bottom row reaches
    neither gq nor gt."""
    c = C.tfm_case(n)
    got = C.run_tfm(_lib.lib(), X, c)
    C.check_tfm(c, got, "gpu")
    q, t = leaf(c["q"]), leaf(c["t"])
    T = transformation_matrix_batch(q, t)
    T.backward(X.dev(c["gT_other_bottom"]))
    np.testing.assert_array_equal(bits(X.host(T.detach())), bits(got["T"]))
    np.testing.assert_array_equal(bits(X.host(q.grad)), bits(got["gq"]))
    np.testing.assert_array_equal(bits(X.host(t.grad)), bits(got["gt"]))


def test_chain_stage_by_stage():
    """epilogue -> transformation matrix -> ADD / ADD-S -> confidence loss as ``Model.loss_device`` composes them, through
    the wrappers and autograd; every intermediate tensor of the graph is kept and each stage is checked on the float32
    tensors the device itself handed to it (losschain_cases.check_chain)."""
    c = C.chain_case()
    B, P, nf, M = c["B"], c["P"], c["nf"], c["M"]
    n = B * P
    orot, otrn, ocnf = leaf(c["orot"]), leaf(c["otrn"]), leaf(c["ocnf"])
    rot, trans, conf = K.PoseEpilogue.apply(orot, otrn, ocnf, X.dev(c["class_id"]), X.dev(c["pts"]), X.dev(c["pitch"]),
                                            X.dev(c["origin"]), B, P, nf)
    T_pred = transformation_matrix_batch(rot.reshape(n, 4), trans.reshape(n, 3)).reshape(B, P, 4, 4)
    T_true = transformation_matrix_batch(X.dev(c["q_true"]), X.dev(c["t_true"]))
    add = average_distance_batch(X.dev(c["points"]), T_true, T_pred, X.dev(c["sym"]).bool())
    loss = confidence_loss(add, conf, c["lam"])
    for t in (rot, trans, conf, T_pred, add):
        t.retain_grad()
    loss.backward()
    # the arg-min rows and cnt are not outputs of the wrappers: the same forward calls through the C ABI
    L, p = _lib.lib(), X.ptr
    idx = X.dev(np.full((B, P, M), C.ISENT, np.int32))
    out2 = torch.empty_like(add)
    pts, sym, Tp_d = X.dev(c["points"]), X.dev(c["sym"]), T_pred.detach().contiguous()
    assert L.mf_average_distance_fwd(p(pts), p(T_true), p(Tp_d), p(sym), B, M, P, p(out2), p(idx), X.stream) == 0
    cnt, loss2 = X.dev(np.full(B, C.ISENT, np.int32)), torch.empty(1, device="cuda")
    add_d, conf_d = add.detach().contiguous(), conf.detach().contiguous()
    assert L.mf_confidence_loss_fwd(p(add_d), p(conf_d), B, P, c["lam"], p(loss2), p(cnt), X.stream) == 0
    X.sync()
    np.testing.assert_array_equal(bits(X.host(out2)), bits(X.host(add_d)))
    h = lambda t: X.host(t.detach())  # noqa: E731
    got = dict(rot=h(rot), trans=h(trans), conf=h(conf), T_pred=h(T_pred), T_true=h(T_true), add=h(add),
               loss=h(loss).reshape(1), idx=h(idx), cnt=h(cnt), dadd=h(add.grad), dconf=h(conf.grad), gT=h(T_pred.grad),
               gq=h(rot.grad).reshape(n, 4), gt=h(trans.grad).reshape(n, 3), drot=h(orot.grad), dtrn=h(otrn.grad),
               dcnf=h(ocnf.grad))
    C.check_chain(c, got, "gpu")
