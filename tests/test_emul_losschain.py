"""The training loss chain's kernel TEXT (csrc/loss.hip, csrc/pointops.hip with quat.h) on the host emulator, through the
C ABI, against the float64 references and a-priori bounds of tests/losschain_ref.py on the cases of
tests/losschain_cases.py (its docstring says which case reaches which branch).  Every output element is compared;
the arg-min rows are checked against the float32 mirror AND, independently, against the float64 minimum; a second call
gives the same bits; and the comparator itself is shown to reject the errors a plausible kernel bug would make, on
NumPy arrays only (the project's code is never broken to show that a test bites)."""
import numpy as np
import pytest

import losschain_cases as C
import losschain_ref as R
from host_emul import emul
from oracle import oracle_np as O

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

X = C.Host


@pytest.fixture(scope="module")
def loss_lib():
    return emul.build(["loss.hip"])


@pytest.fixture(scope="module")
def point_lib():
    return emul.build(["pointops.hip"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    C.report()


# ---- the references stand on their own feet ---------------------------------------------------------------------------
def test_reference_gradients_agree_with_central_differences_and_the_oracle():
    """tests/losschain_ref.py against itself: every analytic gradient against central differences of its own float64
    forward, and the closed-form quaternion gradient against the oracle's chain rule (two derivations)."""
    rs = np.random.RandomState(7)
    q, gT = rs.randn(6, 4) * np.array([[1e-2], [0.3], [1.0], [2.0], [30.0], [1.0]]), rs.randn(6, 4, 4)
    (gq, gt), _ = R.transformation_matrix_grad(q, gT)
    np.testing.assert_allclose(gq, O.quaternion_matrix_backward(q, gT), rtol=1e-9, atol=1e-12)
    num = np.zeros_like(q)
    for k in range(4):
        h = 1e-6 * np.abs(q).max(axis=1)
        dq = np.zeros_like(q)
        dq[:, k] = h
        num[:, k] = ((R.transformation_matrix(q + dq, q[:, :3])[0] - R.transformation_matrix(q - dq, q[:, :3])[0])
                     * gT).sum(axis=(1, 2)) / (2 * h)
    np.testing.assert_allclose(gq, num, rtol=1e-5, atol=1e-7 * np.abs(gq).max())
    np.testing.assert_array_equal(gt, gT[:, :3, 3])
    np.testing.assert_allclose(R.transformation_matrix(q, q[:, :3])[0], O.transformation_matrix(q, q[:, :3]), rtol=1e-12,
                               atol=1e-14)
    c = C.add_case(37)
    idx = C.add_mirror(37)
    gT_, _ = R.average_distance_grad(c["points"], c["T_true"], c["T_pred"], c["sym"], idx, c["gout"])
    for b, p in ((0, 1), (1, 2), (2, 0)):
        for i, j in ((0, 0), (1, 3), (2, 1)):
            v = []
            for sgn in (1, -1):
                Tp = c["T_pred"].astype(np.float64).copy()
                Tp[b, p, i, j] += sgn * 1e-7
                v.append(np.nansum(R.average_distance(c["points"], c["T_true"], Tp, c["sym"], idx=idx)[0] * c["gout"]))
            np.testing.assert_allclose(gT_[b, p, i, j], (v[0] - v[1]) / 2e-7, rtol=1e-5, atol=1e-9)
    cc = C.conf_case(3, 63)
    (dadd, dconf), _ = R.confidence_loss_grad(cc["add"], cc["conf"], cc["lam"], 1.0)
    for arr, name in ((dadd, "add"), (dconf, "conf")):
        for b, p in ((0, int(np.argmax(cc["conf"][0] > 0))), (2, int(np.argmax(cc["conf"][2] > 0)))):
            v = []
            for sgn in (1, -1):
                a = {k: cc[k].astype(np.float64).copy() for k in ("add", "conf")}
                a[name][b, p] += sgn * 1e-7
                v.append(R.confidence_loss(a["add"], a["conf"], cc["lam"])[0])
            np.testing.assert_allclose(arr[b, p], (v[0] - v[1]) / 2e-7, rtol=1e-5)
    e = C.epi_case(5, 13, 3)
    live = np.nan_to_num
    (drot, dtrn, dcnf), _ = R.pose_epilogue_grad(e["orot"], e["ocnf"], e["class_id"], e["pitch"], e["grot"], e["gtrans"],
                                                 e["gconf"], 3)

    def phi(orot, otrn, ocnf):
        (r, t, cf), _ = R.pose_epilogue(orot, otrn, ocnf, e["class_id"], e["pts"], e["origin"], e["pitch"], 3)
        return (live(r * e["grot"]).sum() + live(t * e["gtrans"]).sum() + live(cf * e["gconf"]).sum())
    for name, arr, (row, col) in (("orot", drot, (15, 5)), ("orot", drot, (3, 2)), ("otrn", dtrn, (14, 4)), ("ocnf", dcnf, (60, 1))):
        v = []
        for sgn in (1, -1):
            a = {k: e[k].astype(np.float64).copy() for k in ("orot", "otrn", "ocnf")}
            a[name][row, col] += sgn * 1e-6
            v.append(phi(a["orot"], a["otrn"], a["ocnf"]))
        np.testing.assert_allclose(arr[row, col], (v[0] - v[1]) / 2e-6, rtol=1e-5, atol=1e-9)


def test_case_1025_tail_point_alone_in_its_tile_is_a_unique_nearest_neighbour():
    C.assert_tail_point_is_a_unique_neighbour(1025)


# ---- the kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", C.ADD_MS)
def test_add_adds_every_element_within_its_bound(loss_lib, M):
    """loss_walk forward and backward (with the forward's indices): M < 4, M = 1, one tile staged once (M <= 1024), the
    unstaged multi-tile search (M = 1025: a last tile of one point padded with +inf; 2051), more than one round with a
    ragged last one, ties between tiles and inside a group of four, the n > 0 guard (pose [0, 0]) and grp == -1 (the
    NaN pose [2, 1])."""
    c = C.add_case(M)
    got = C.run_add(loss_lib, X, c)
    C.check_add(c, got, "emul")
    assert (got["idx"][0] == C.ISENT).all()   # ADD rows of nn_idx are not written
    again = C.run_add(loss_lib, X, c)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), again[k].view(np.int32))


@pytest.mark.parametrize("M", [300, 1025, 2051])
def test_add_backward_that_repeats_the_search_gives_the_same_bits(loss_lib, M):
    """nn_idx = NULL in the backward (C ABI only): the search is repeated, within one tile (300) and across tiles with
    the tile restaged every round (1025, 2051); bit-equal to the backward on the forward's indices, and the forward's
    value does not depend on whether it keeps the indices."""
    c = C.add_case(M)
    a = C.run_add(loss_lib, X, c, bwd_idx=True)
    b = C.run_add(loss_lib, X, c, bwd_idx=False)
    np.testing.assert_array_equal(a["gT"].view(np.int32), b["gT"].view(np.int32))
    n = C.run_add(loss_lib, X, c, bwd_idx=False, fwd_idx=False)
    np.testing.assert_array_equal(a["out"].view(np.int32), n["out"].view(np.int32))
    np.testing.assert_array_equal(a["gT"].view(np.int32), n["gT"].view(np.int32))
    if M == 300:
        C.check_add(c, a, "emul")


@pytest.mark.parametrize("B,P", C.CONF_SHAPES)
def test_confidence_loss_every_element_within_its_bound(loss_lib, B, P):
    """k_conf_loss_fwd / _bwd: P < 64, a wave's second object (B > 16), a lane's second round (P > 64), conf == 0
    exactly, and at (40, 65) object 23 (wave 7, second pass) without a confident point: cnt = 0, NaN total, zero rows."""
    c = C.conf_case(B, P)
    got = C.run_conf(loss_lib, X, c)
    C.check_conf(c, got, "emul")
    again = C.run_conf(loss_lib, X, c)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), again[k].view(np.int32))
    if (B, P) == (40, 65):
        assert got["cnt"][23] == 0 and np.isnan(got["loss"][0])
        f = C.conf_case(B, P, finite=True)
        C.check_conf(f, C.run_conf(loss_lib, X, f), "emul")


def test_confidence_loss_refuses_b_0_and_b_8193(loss_lib):
    C.check_conf_refusals(loss_lib, X)


@pytest.mark.parametrize("B,P,nf", C.EPI_SHAPES)
def test_pose_epilogue_every_element_within_its_bound(point_lib, B, P, nf):
    """k_pose_epi3_fwd / _bwd: n_fg = 1, B P 8 n_fg not a multiple of 256, the first and the last class, ids 0 and
    n_fg + 1 (NaN forward, rows of zeros backward over a sentinel, NaN cotangents), s == 0 and a row of norm 1e-6."""
    c = C.epi_case(B, P, nf)
    assert (B * P * 8 * nf) % 256
    got = C.run_epi(point_lib, X, c)
    C.check_epi(c, got, "emul")
    again = C.run_epi(point_lib, X, c)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), again[k].view(np.int32))


@pytest.mark.parametrize("n", C.TFM_NS)
def test_transformation_matrix_every_element_within_its_bound(point_lib, n):
    """k_tfm_fwd / _bwd around a block boundary, quaternion norms 1e-3 .. 1e3; the cotangent's bottom row reaches
    neither gq nor gt."""
    c = C.tfm_case(n)
    got = C.run_tfm(point_lib, X, c)
    C.check_tfm(c, got, "emul")
    other = C.run_tfm(point_lib, X, c, gT="gT_other_bottom")
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), other[k].view(np.int32))


def test_chain_stage_by_stage():
    lib = emul.build(["loss.hip", "pointops.hip"])
    c = C.chain_case()
    got = C.run_chain(lib, X, c)
    C.check_chain(c, got, "emul")
    assert not any((np.asarray(v) == C.SENT).any() for k, v in got.items() if v.dtype == np.float32)


# ---- the comparator bites: plausible kernel bugs, applied to the REFERENCE's own output -----------------------------------
def _reference_result(M):
    c = C.add_case(M)
    idx = C.add_mirror(M).astype(np.int32)
    args = (c["points"], c["T_true"], c["T_pred"], c["sym"])
    return c, dict(out=R.average_distance(*args, idx=idx)[0], idx=idx,
                   gT=R.average_distance_grad(*args, idx, c["gout"])[0])


def _recomputed(c, idx):
    args = (c["points"], c["T_true"], c["T_pred"], c["sym"])
    return dict(out=R.average_distance(*args, idx=idx)[0], idx=idx, gT=R.average_distance_grad(*args, idx, c["gout"])[0])


def test_comparator_accepts_the_reference_and_rejects_add_corruptions():
    c, ref = _reference_result(1025)
    M = 1025
    C.check_add(c, ref, "self")
    # (1) the second-nearest index for one query (value and gradient consistent with it)
    b, p = 1, 1
    pts = c["points"][b].astype(np.float64)
    true = R._images(pts, c["T_true"][b].astype(np.float64))[0]
    pred = R._images(pts, c["T_pred"][b, p].astype(np.float64))[0]
    ssd = ((true[:, None] - pred[None]) ** 2).sum(axis=2)
    order = np.argsort(ssd, axis=0, kind="stable")
    m = int(np.argmax(ssd[order[1], np.arange(M)] - ssd[order[0], np.arange(M)]))
    idx = ref["idx"].copy()
    idx[b, p, m] = order[1, m]
    bad = _recomputed(c, idx)
    with pytest.raises(AssertionError, match="float32 mirror"):
        C.check_indices(c, bad["idx"], "corrupt")
    diff, bnd = R.argmin_slack(c["points"][b], c["T_true"][b], c["T_pred"][b, p], idx[b, p])
    assert diff[m] > bnd[m] and (np.delete(diff, m) <= np.delete(bnd, m)).all()   # the independent float64 check
    sref, sbound, _ = C._add_search(M)
    assert not R.compare(bad["out"], sref, sbound)[0]
    # (2) the tail point (alone in its tile) dropped from the mean and from the gradient sums
    n_tail, g_tail = np.zeros((c["B"], c["P"])), np.zeros((c["B"], c["P"], 4, 4))
    for bb in range(c["B"]):
        for pp in range(c["P"]):
            k = ref["idx"][bb, pp, M - 1] if c["sym"][bb] else M - 1
            x = c["points"][bb].astype(np.float64)
            d = (R._images(x, c["T_true"][bb].astype(np.float64))[0][k]
                 - R._images(x, c["T_pred"][bb, pp].astype(np.float64))[0][M - 1])
            n_tail[bb, pp] = np.linalg.norm(d)
            if n_tail[bb, pp] > 0:
                g_tail[bb, pp, :3] = -c["gout"][bb, pp] / M * np.outer(d / n_tail[bb, pp], np.r_[x[M - 1], 1.0])
    bad = dict(ref, out=ref["out"] - n_tail / M)
    with pytest.raises(AssertionError, match="value"):
        C.check_add(c, bad, "corrupt")
    bad = dict(ref, gT=ref["gT"] - g_tail)
    with pytest.raises(AssertionError, match="gradient"):
        C.check_add(c, bad, "corrupt")
    # (3) the later copy of a tied pair: same distance, same value -- only the index rule can tell
    idx = ref["idx"].copy()
    hit = np.argwhere(idx == 12)
    assert len(hit)
    idx[tuple(hit[0])] = M - 20 + 2
    assert np.array_equal(c["points"][:, 12], c["points"][:, M - 18])
    with pytest.raises(AssertionError, match="float32 mirror"):
        C.check_add(c, dict(ref, idx=idx), "corrupt")


def test_comparator_rejects_confidence_and_epilogue_corruptions():
    c = C.conf_case(40, 65)
    loss, _, cnt = R.confidence_loss(c["add"], c["conf"], c["lam"])
    (dadd, dconf), _ = R.confidence_loss_grad(c["add"], c["conf"], c["lam"], c["gloss"][0])
    ref = dict(loss=np.array([loss]), cnt=cnt, dadd=dadd, dconf=dconf)
    C.check_conf(c, ref, "self")
    # object 23's count taken from object 7 (a wave that does not reset between its two passes)
    bad_cnt = cnt.copy()
    bad_cnt[23] = cnt[7]
    with pytest.raises(AssertionError, match="confident points"):
        C.check_conf(c, dict(ref, cnt=bad_cnt), "corrupt")
    assert cnt[7] != cnt[8]
    scaled = dadd.copy()
    scaled[7] *= cnt[7] / cnt[8]   # object 7's gradient divided by its neighbour's count
    with pytest.raises(AssertionError, match="dadd"):
        C.check_conf(c, dict(ref, dadd=scaled), "corrupt")
    f = C.conf_case(40, 65, finite=True)
    loss, _, cnt = R.confidence_loss(f["add"], f["conf"], f["lam"])
    (dadd, dconf), _ = R.confidence_loss_grad(f["add"], f["conf"], f["lam"], f["gloss"][0])
    ref = dict(loss=np.array([loss]), cnt=cnt, dadd=dadd, dconf=dconf)
    C.check_conf(f, ref, "self")
    term = f["add"][23, 64].astype(np.float64) * 0.25 - float(np.float32(f["lam"])) * np.log(0.25)
    with pytest.raises(AssertionError, match="loss"):   # the second round's point (lane 0, p = 64) dropped from the sum
        C.check_conf(f, dict(ref, loss=np.array([loss - term / 40])), "corrupt")
    # a class column shifted by one
    e = C.epi_case(5, 13, 3)
    fw, _ = R.pose_epilogue(e["orot"], e["otrn"], e["ocnf"], e["class_id"], e["pts"], e["origin"], e["pitch"], 3)
    bw, _ = R.pose_epilogue_grad(e["orot"], e["ocnf"], e["class_id"], e["pitch"], e["grot"], e["gtrans"], e["gconf"], 3)
    ref = dict(zip(("rot", "trans", "conf", "drot", "dtrn", "dcnf"), fw + bw))
    C.check_epi(e, ref, "self")
    for k, w in (("drot", 4), ("dtrn", 3), ("dcnf", 1)):
        with pytest.raises(AssertionError, match=k):
            C.check_epi(e, dict(ref, **{k: np.roll(ref[k], w, axis=1)}), "corrupt")
    shifted = e["class_id"].copy()
    shifted[4] = 3   # object 4 (class 2) read from the next class's columns
    fw2, _ = R.pose_epilogue(e["orot"], e["otrn"], e["ocnf"], shifted, e["pts"], e["origin"], e["pitch"], 3)
    for k, v in zip(("rot", "trans", "conf"), fw2):
        with pytest.raises(AssertionError, match=k):
            C.check_epi(e, dict(ref, **{k: v}), "corrupt")
    left = ref["drot"].copy()
    left[5 * 13 - 1, :] = C.SENT   # the last row left as allocated
    with pytest.raises(AssertionError, match="unwritten"):
        C.check_epi(e, dict(ref, drot=left), "corrupt")
