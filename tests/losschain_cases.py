"""TEST INFRASTRUCTURE: the cases of the training loss chain, shared by tests/test_emul_losschain.py (kernel text on the
host emulator) and tests/test_gpu_losschain.py (the MI355X), with the code that runs them through the C ABI and checks
the results against tests/losschain_ref.py.  Seeded, small: each case is the smallest shape at which its branch of
csrc/loss.hip / csrc/pointops.hip is live.

ADD / ADD-S (``add_case(M)``: B = 3, symmetric = [0, 1, 1], P = 3; loss_walk):
  M = 1, 3 (M < 4: the +inf padding of the only group), 4, 5, 255, 256, 257 (a second round with one live lane),
  1023, 1024 (the largest staged model), 1025 (unstaged multi-tile search, a last tile of ONE point padded with +inf),
  2051 (three tiles, nine rounds, M not a multiple of 256 or 4).
  pose [0, 0] equals the true pose bit for bit          -> value exactly 0, gradient rows exactly 0 (the n > 0 guard)
  pose [1, 0] is the true pose moved by 0.1 mm          -> every query's neighbour is its own point; at M = 1025 the
                                                           tail point, alone in its tile, is a unique nearest neighbour
  pose [2, 1] has a NaN translation component           -> grp == -1: no candidate beats +inf; value NaN, index row 0
  M >= 257: points 10 .. 19 are copies of M-20 .. M-11  -> exact ties, beyond M = 1024 between two tiles: the earlier
                                                           tile wins; point 42 copies 41: a tie inside a group of four
Confidence loss (``conf_case``): (B, P) = (1, 1), (3, 63) (P < 64), (17, 64) (wave 0 takes a second object), (40, 65)
  (a second round of one lane; object 23 = wave 7's second pass has no positive entry: cnt = 0, NaN), (33, 130);
  conf = rand - 0.2 with entries exactly 0.
Pose epilogue (``epi_case``): (B, P, n_fg) = (1, 1, 1), (3, 5, 1), (2, 37, 21), (5, 13, 3); class ids 1, n_fg, 0 and
  n_fg + 1, an all-zero quaternion row (s == 0) and one of norm 1e-6, NaN cotangents for the objects without a head.
Transformation matrix (``tfm_case``): n = 1, 255, 256, 257; quaternion norms 1e-3 .. 1e3; cotangents with a bottom row.
The chain (``chain_case``): B = 3, P = 5, n_fg = 3, M = 37, object 1 symmetric, checked stage by stage.
"""
import functools

import numpy as np

import losschain_ref as R
from oracle import oracle_np as O

SENT = np.float32(-12345.0)   # pre-fill of every output buffer: an unwritten element shows
ISENT = -7
ADD_MS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2051)
CONF_SHAPES = ((1, 1), (3, 63), (17, 64), (40, 65), (33, 130))
EPI_SHAPES = ((1, 1, 1), (3, 5, 1), (2, 37, 21), (5, 13, 3))
TFM_NS = (1, 255, 256, 257)
LAM = 0.015
INVALID = -1                  # -hipErrorInvalidValue, the refusal code of include/mfhip.h

f32 = np.float32


class Host:
    """NumPy arrays as device memory (the emulator).  The GPU test has a torch twin."""
    @staticmethod
    def dev(a):
        return np.ascontiguousarray(a).copy()

    @staticmethod
    def host(a):
        return a

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    stream = None

    @staticmethod
    def sync():
        pass


# ---- ADD / ADD-S ----------------------------------------------------------------------------------------------------
def _poses(rs, n):
    """As ``_poses`` of tests/test_gpu_training.py."""
    from morefusion_amd.synthetic import random_rotation
    T = np.tile(np.eye(4, dtype=f32), (n, 1, 1))
    for k in range(n):
        T[k, :3, :3] = random_rotation(rs, 0.8)
        T[k, :3, 3] = rs.uniform(-0.05, 0.05, 3)
    return T


@functools.lru_cache(maxsize=None)
def add_case(M):
    from morefusion_amd.synthetic import random_rotation
    rs = np.random.RandomState(1000 + M)
    B, P = 3, 3
    pts = rs.uniform(-0.06, 0.06, (B, M, 3)).astype(f32)
    if M >= 257:
        pts[:, 10:20] = pts[:, M - 20:M - 10]
        pts[:, 42] = pts[:, 41]
    Tt = _poses(rs, B)
    Tp = np.tile(np.eye(4, dtype=f32), (B, P, 1, 1))
    for b in range(B):
        for p in range(P):
            Tp[b, p, :3, :3] = (Tt[b, :3, :3].astype(np.float64) @ random_rotation(rs, 0.05)).astype(f32)
            Tp[b, p, :3, 3] = Tt[b, :3, 3] + rs.uniform(-0.01, 0.01, 3).astype(f32)
    Tp[0, 0] = Tt[0]
    Tp[1, 0] = Tt[1]
    Tp[1, 0, :3, 3] += np.array([1e-4, -1e-4, 1e-4], f32)
    Tp[2, 1, 1, 3] = np.nan
    case = dict(M=M, B=B, P=P, points=pts, T_true=Tt, T_pred=Tp, sym=np.array([0, 1, 1], np.uint8),
                gout=rs.uniform(0.5, 1.5, (B, P)).astype(f32))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def add_mirror(M):
    """The float32 mirror's arg-min rows (oracle_np.nn on the float32 images, lowest index among equal float32 squared
    distances; 0 for a NaN query): what the contract gives, [B,P,M], -7 in the rows of ADD objects."""
    c = add_case(M)
    want = np.full((c["B"], c["P"], M), ISENT, np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(c["B"]):
            if c["sym"][b]:
                pt = O.transform_points(c["points"][b], c["T_true"][b])
                pp = O.transform_points(c["points"][b], c["T_pred"][b])
                want[b] = O.nn(pt, pp.reshape(-1, 3)).reshape(c["P"], M)
    return want


def run_add(lib, X, c, bwd_idx=True, fwd_idx=True):
    B, M, P = c["B"], c["M"], c["P"]
    pts, Tt, Tp, sym, gout = (X.dev(c[k]) for k in ("points", "T_true", "T_pred", "sym", "gout"))
    out = X.dev(np.full((B, P), SENT, f32))
    idx = X.dev(np.full((B, P, M), ISENT, np.int32))
    gT = X.dev(np.full((B, P, 4, 4), SENT, f32))
    assert lib.mf_average_distance_fwd(X.ptr(pts), X.ptr(Tt), X.ptr(Tp), X.ptr(sym), B, M, P, X.ptr(out),
                                       X.ptr(idx) if fwd_idx else None, X.stream) == 0
    assert lib.mf_average_distance_bwd(X.ptr(pts), X.ptr(Tt), X.ptr(Tp), X.ptr(sym), X.ptr(gout), B, M, P,
                                       X.ptr(idx) if bwd_idx else None, X.ptr(gT), X.stream) == 0
    X.sync()
    return dict(out=X.host(out), idx=X.host(idx), gT=X.host(gT))


def check_indices(c, idx, tag):
    """The arg-min rows: bit-equal to the float32 mirror; never the later copy of a tie; and, independently of the
    mirror, near-optimal in float64 for EVERY pair (a NaN query must give 0)."""
    M = c["M"]
    idx = np.asarray(idx)
    want = add_mirror(M)
    assert idx.shape == want.shape
    bad = np.argwhere(idx != want)
    assert len(bad) == 0, (tag, "arg-min differs from the float32 mirror at (b, p, m)", bad[:5].tolist(),
                           idx[tuple(bad[0])], want[tuple(bad[0])])
    worst = 0.0
    for b in range(c["B"]):
        if not c["sym"][b]:
            continue
        assert idx[b].min() >= 0 and idx[b].max() < M
        if M >= 257:
            assert not np.isin(idx[b], np.r_[M - 20:M - 10, 42]).any(), (tag, "the later copy of a tie was chosen")
        for p in range(c["P"]):
            diff, bnd = R.argmin_slack(c["points"][b], c["T_true"][b], c["T_pred"][b, p], idx[b, p])
            nanq = np.isnan(bnd)
            assert (idx[b, p][nanq] == 0).all(), (tag, "a NaN query must give index 0")
            assert (diff[~nanq] <= bnd[~nanq]).all(), (tag, b, p, "choice farther than the float64 minimum allows")
            if (~nanq).any() and (diff[~nanq] > 0).any():
                worst = max(worst, float((diff[~nanq] / bnd[~nanq]).max()))
    return worst


def check_add(c, got, tag):
    """Everything about one ADD / ADD-S result: indices, values against the float64 reference with the result's own
    (verified) indices and against the float64 search, gradients, the exact zeros and the NaN pose."""
    M, B, P = c["M"], c["B"], c["P"]
    out, idx, gT = (np.asarray(got[k]) for k in ("out", "idx", "gT"))
    check_indices(c, idx, tag)
    args = (c["points"], c["T_true"], c["T_pred"], c["sym"])
    ref, bound, _ = R.average_distance(*args, idx=idx)
    R.assert_within(out, ref, bound, f"{tag} add M={M} value (frozen idx)", op=f"{tag} add value")
    sref, sbound, sidx = _add_search(M)
    extra = np.zeros((B, P))
    for b in range(B):
        for p in range(P):
            if c["sym"][b] and not np.isnan(sref[b, p]) and (sidx[b, p] != idx[b, p]).any():
                _, bnd = R.argmin_slack(c["points"][b], c["T_true"][b], c["T_pred"][b, p], idx[b, p])
                extra[b, p] = np.sqrt(bnd[sidx[b, p] != idx[b, p]]).sum() / M   # n_got - n_min <= sqrt(ssd_got - ssd_min)
    R.assert_within(out, sref, sbound + extra, f"{tag} add M={M} value (float64 search)", op=f"{tag} add value")
    assert out[0, 0] == 0.0, (tag, "pose equal to the truth bit for bit", out[0, 0])
    assert np.isnan(out[2, 1]) and (idx[2, 1] == 0).all(), (tag, "NaN pose")
    gref, gbound = R.average_distance_grad(*args, idx, c["gout"])
    R.assert_within(gT, gref, gbound, f"{tag} add M={M} gradient", op=f"{tag} add gradient")
    assert (gT[:, :, 3] == 0).all(), (tag, "row 3 of the gradient")
    assert (gT[0, 0] == 0).all(), (tag, "zero residual: gradient rows exactly 0, not NaN", gT[0, 0])
    assert (gT[2, 1] == 0).all(), (tag, "NaN pose: gradient rows are zeros (include/mfhip.h)")
    assert np.isfinite(np.delete(out.ravel(), 2 * P + 1)).all() and np.isfinite(gT).all()


@functools.lru_cache(maxsize=None)
def _add_search(M):
    c = add_case(M)
    return R.average_distance(c["points"], c["T_true"], c["T_pred"], c["sym"], idx=None)


def assert_tail_point_is_a_unique_neighbour(M=1025):
    """On the REFERENCE: in the case M = 1025 the last point (alone in the second tile) is the nearest true point of
    query M - 1 under pose [1, 0], and every other candidate is farther by more than float32 can blur."""
    c = add_case(M)
    b, p, m = 1, 0, M - 1
    pts = c["points"][b].astype(np.float64)
    true, Ct = R._images(pts, c["T_true"][b].astype(np.float64))
    pred, Cp = R._images(pts, c["T_pred"][b, p].astype(np.float64))
    d = true - pred[m]
    ssd = (d * d).sum(axis=1)
    pb = R.pair_bound(d, 5 * R.U * (Ct + Cp[m]))
    assert int(ssd.argmin()) == m
    others = np.delete(np.arange(M), m)
    assert (ssd[others] - ssd[m] > pb[others] + pb[m]).all()
    assert add_mirror(M)[b, p, m] == m


# ---- confidence loss ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conf_case(B, P, finite=False):
    """``finite``: object 23 of (40, 65) gets one positive entry (its last point: lane 0's second round), so that the
    sums of that shape are checked as values too."""
    rs = np.random.RandomState(2000 + 131 * B + P)
    add = rs.uniform(0.0, 0.05, (B, P)).astype(f32)
    conf = (rs.rand(B, P) - 0.2).astype(f32)
    if B * P >= 8:
        conf.flat[rs.choice(B * P, B * P // 8, replace=False)] = 0.0
    else:
        conf[:] = 0.37
    for b in range(B):
        if not (conf[b] > 0).any():
            conf[b, 0] = 0.5
    if (B, P) == (40, 65):
        conf[23] = -np.abs(conf[23])
        if finite:
            conf[23, 64] = 0.25
    return dict(B=B, P=P, add=add, conf=conf, lam=LAM, gloss=np.array([1.7], f32))


def run_conf(lib, X, c):
    B, P = c["B"], c["P"]
    add, conf, gloss = X.dev(c["add"]), X.dev(c["conf"]), X.dev(c["gloss"])
    loss = X.dev(np.full(1, SENT, f32))
    cnt = X.dev(np.full(B, ISENT, np.int32))
    dadd, dconf = X.dev(np.full((B, P), SENT, f32)), X.dev(np.full((B, P), SENT, f32))
    assert lib.mf_confidence_loss_fwd(X.ptr(add), X.ptr(conf), B, P, c["lam"], X.ptr(loss), X.ptr(cnt), X.stream) == 0
    assert lib.mf_confidence_loss_bwd(X.ptr(add), X.ptr(conf), X.ptr(cnt), X.ptr(gloss), B, P, c["lam"], X.ptr(dadd),
                                      X.ptr(dconf), X.stream) == 0
    X.sync()
    return dict(loss=X.host(loss), cnt=X.host(cnt), dadd=X.host(dadd), dconf=X.host(dconf))


def check_conf(c, got, tag):
    B, P = c["B"], c["P"]
    ref, bound, cnt = R.confidence_loss(c["add"], c["conf"], c["lam"])
    assert np.array_equal(np.asarray(got["cnt"]), cnt), (tag, "confident points per object", got["cnt"], cnt)
    assert (c["conf"] == 0).any() or B * P < 8
    R.assert_within(np.asarray(got["loss"]).reshape(()), np.asarray(ref), np.asarray(bound), f"{tag} conf ({B},{P}) loss",
                    op=f"{tag} conf loss")
    (dadd, dconf), (ba, bc) = R.confidence_loss_grad(c["add"], c["conf"], c["lam"], c["gloss"][0])
    R.assert_within(got["dadd"], dadd, ba, f"{tag} conf ({B},{P}) dadd", op=f"{tag} conf gradient")
    R.assert_within(got["dconf"], dconf, bc, f"{tag} conf ({B},{P}) dconf", op=f"{tag} conf gradient")
    if (cnt == 0).any():
        assert np.isnan(ref) and np.isnan(np.asarray(got["loss"])).all()
        dead = cnt == 0
        assert (np.asarray(got["dadd"])[dead] == 0).all() and (np.asarray(got["dconf"])[dead] == 0).all()
        assert np.isfinite(np.asarray(got["dadd"])).all() and np.isfinite(np.asarray(got["dconf"])).all()
        assert np.abs(np.asarray(got["dconf"])[~dead]).max() > 0
    else:
        assert np.isfinite(ref)


def check_conf_refusals(lib, X):
    """B = 8193 and B = 0 are host-side argument checks of mf_confidence_loss_fwd (csrc/loss.hip: they return before the
    launch): the stated code, and no output is touched."""
    add, conf = X.dev(np.ones((4, 4), f32)), X.dev(np.ones((4, 4), f32))
    for B in (8193, 0):
        loss, cnt = X.dev(np.full(1, SENT, f32)), X.dev(np.full(4, ISENT, np.int32))
        assert lib.mf_confidence_loss_fwd(X.ptr(add), X.ptr(conf), B, 1, LAM, X.ptr(loss), X.ptr(cnt), X.stream) == INVALID
        X.sync()
        assert X.host(loss)[0] == SENT and (X.host(cnt) == ISENT).all()


# ---- pose epilogue ----------------------------------------------------------------------------------------------------
EPI_CLASS_IDS = {(1, 1, 1): [1], (3, 5, 1): [1, 0, 2], (2, 37, 21): [21, 1], (5, 13, 3): [1, 3, 0, 4, 2]}


@functools.lru_cache(maxsize=None)
def epi_case(B, P, nf):
    rs = np.random.RandomState(3000 + 97 * B + 7 * P + nf)
    n = B * P
    cid = np.array(EPI_CLASS_IDS[(B, P, nf)], np.int64)
    orot = (rs.randn(n, 4 * nf) * 1.5).astype(f32)
    if P >= 2:   # rows 0 and 1 belong to object 0 (class 1 or n_fg: live)
        fg = int(cid[0]) - 1
        orot[0, 4 * fg:4 * fg + 4] = 0.0
        v = orot[1, 4 * fg:4 * fg + 4].astype(np.float64)
        orot[1, 4 * fg:4 * fg + 4] = (v / np.linalg.norm(v) * 1e-6).astype(f32)
    c = dict(B=B, P=P, nf=nf, class_id=cid, orot=orot, otrn=rs.randn(n, 3 * nf).astype(f32),
             ocnf=(rs.randn(n, nf) * 2).astype(f32), pts=rs.uniform(0, 32, (n, 3)).astype(f32),
             origin=rs.uniform(-0.5, 0.5, (B, 3)).astype(f32), pitch=rs.uniform(0.004, 0.01, B).astype(f32),
             grot=rs.randn(B, P, 4).astype(f32), gtrans=rs.randn(B, P, 3).astype(f32), gconf=rs.randn(B, P).astype(f32))
    for b in range(B):   # an object without a head: its forward is NaN, so are the cotangents that come back
        if not 1 <= cid[b] <= nf:
            c["grot"][b], c["gtrans"][b], c["gconf"][b] = np.nan, np.nan, np.nan
    return c


def run_epi(lib, X, c):
    B, P, nf = c["B"], c["P"], c["nf"]
    n = B * P
    d = {k: X.dev(c[k]) for k in ("orot", "otrn", "ocnf", "class_id", "pts", "origin", "pitch", "grot", "gtrans", "gconf")}
    o = {k: X.dev(np.full(s, SENT, f32)) for k, s in (("rot", (B, P, 4)), ("trans", (B, P, 3)), ("conf", (B, P)),
                                                       ("drot", (n, 4 * nf)), ("dtrn", (n, 3 * nf)), ("dcnf", (n, nf)))}
    p = X.ptr
    assert lib.mf_pose_epilogue_train_fwd(p(d["orot"]), p(d["otrn"]), p(d["ocnf"]), p(d["class_id"]), p(d["pts"]),
                                          p(d["origin"]), p(d["pitch"]), B, P, nf, p(o["rot"]), p(o["trans"]),
                                          p(o["conf"]), X.stream) == 0
    assert lib.mf_pose_epilogue_train_bwd(p(d["orot"]), p(d["ocnf"]), p(d["class_id"]), p(d["pitch"]), p(d["grot"]),
                                          p(d["gtrans"]), p(d["gconf"]), B, P, nf, p(o["drot"]), p(o["dtrn"]),
                                          p(o["dcnf"]), X.stream) == 0
    X.sync()
    return {k: X.host(v) for k, v in o.items()}


def check_epi(c, got, tag):
    what = f"{tag} epilogue ({c['B']},{c['P']},{c['nf']})"
    ref, bnd = R.pose_epilogue(c["orot"], c["otrn"], c["ocnf"], c["class_id"], c["pts"], c["origin"], c["pitch"], c["nf"])
    for k, r, b in zip(("rot", "trans", "conf"), ref, bnd):
        R.assert_within(got[k], r, b, f"{what} {k}", op=f"{tag} epilogue forward")
    gref, gbnd = R.pose_epilogue_grad(c["orot"], c["ocnf"], c["class_id"], c["pitch"], c["grot"], c["gtrans"], c["gconf"],
                                      c["nf"])
    for k, r, b in zip(("drot", "dtrn", "dcnf"), gref, gbnd):
        g = np.asarray(got[k])
        assert not (g == SENT).any(), (what, k, "an element was left unwritten")
        R.assert_within(g, r, b, f"{what} {k}", op=f"{tag} epilogue gradient")
    if c["P"] >= 2:   # the all-zero quaternion row: zeros forward, g / 1e-5 backward
        fg = int(c["class_id"][0]) - 1
        assert (np.asarray(got["rot"])[0, 0] == 0).all()
        np.testing.assert_allclose(np.asarray(got["drot"])[0, 4 * fg:4 * fg + 4], c["grot"][0, 0].astype(np.float64) / 1e-5,
                                   rtol=11 * R.U)


# ---- transformation matrix ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tfm_case(n):
    rs = np.random.RandomState(4000 + n)
    q = rs.randn(n, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** np.linspace(-3, 3, n)[rs.permutation(n)][:, None]
    if n >= 2:
        assert np.linalg.norm(q, axis=1).min() < 1.1e-3 and np.linalg.norm(q, axis=1).max() > 0.9e3
    gT = rs.randn(n, 4, 4).astype(f32)
    gT2 = gT.copy()
    gT2[:, 3] = rs.randn(n, 4).astype(f32) * 100
    return dict(n=n, q=q.astype(f32), t=rs.randn(n, 3).astype(f32), gT=gT, gT_other_bottom=gT2)


def run_tfm(lib, X, c, gT="gT"):
    n = c["n"]
    q, t, g = X.dev(c["q"]), X.dev(c["t"]), X.dev(c[gT])
    T, gq, gt = (X.dev(np.full(s, SENT, f32)) for s in ((n, 4, 4), (n, 4), (n, 3)))
    assert lib.mf_transformation_matrix_fwd(X.ptr(q), X.ptr(t), n, X.ptr(T), X.stream) == 0
    assert lib.mf_transformation_matrix_bwd(X.ptr(q), X.ptr(g), n, X.ptr(gq), X.ptr(gt), X.stream) == 0
    X.sync()
    return dict(T=X.host(T), gq=X.host(gq), gt=X.host(gt))


def check_tfm(c, got, tag):
    what = f"{tag} tfm n={c['n']}"
    T, bT = R.transformation_matrix(c["q"], c["t"])
    R.assert_within(got["T"], T, bT, f"{what} T", op=f"{tag} tfm forward")
    (gq, gt), (bq, bt) = R.transformation_matrix_grad(c["q"], c["gT"])
    R.assert_within(got["gq"], gq, bq, f"{what} gq", op=f"{tag} tfm gradient")
    R.assert_within(got["gt"], gt, bt, f"{what} gt", op=f"{tag} tfm gradient")


# ---- the chain --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case():
    rs = np.random.RandomState(5000)
    B, P, nf, M = 3, 5, 3, 37
    n = B * P
    qt = rs.randn(B, 4)
    return dict(B=B, P=P, nf=nf, M=M, class_id=np.array([2, 1, 3], np.int64), sym=np.array([0, 1, 0], np.uint8),
                orot=rs.randn(n, 4 * nf).astype(f32), otrn=(rs.randn(n, 3 * nf) * 2).astype(f32),
                ocnf=rs.randn(n, nf).astype(f32), pts=rs.uniform(0, 32, (n, 3)).astype(f32),
                origin=rs.uniform(-0.3, 0.3, (B, 3)).astype(f32), pitch=rs.uniform(0.004, 0.01, B).astype(f32),
                points=rs.uniform(-0.06, 0.06, (B, M, 3)).astype(f32),
                q_true=(qt / np.linalg.norm(qt, axis=1, keepdims=True)).astype(f32),
                t_true=rs.uniform(-0.3, 0.3, (B, 3)).astype(f32), lam=LAM)


def run_chain(lib, X, c):
    """epilogue -> transformation matrix -> ADD / ADD-S -> confidence loss and back, as ``Model.loss_device`` composes
    them, through the C ABI; every intermediate tensor is returned."""
    B, P, nf, M = c["B"], c["P"], c["nf"], c["M"]
    n = B * P
    p = X.ptr
    d = {k: X.dev(c[k]) for k in ("orot", "otrn", "ocnf", "class_id", "pts", "origin", "pitch", "points", "q_true",
                                  "t_true", "sym")}
    shapes = dict(rot=(B, P, 4), trans=(B, P, 3), conf=(B, P), T_pred=(B, P, 4, 4), T_true=(B, 4, 4), add=(B, P),
                  loss=(1,), dadd=(B, P), dconf=(B, P), gT=(B, P, 4, 4), gq=(n, 4), gt=(n, 3), drot=(n, 4 * nf),
                  dtrn=(n, 3 * nf), dcnf=(n, nf))
    o = {k: X.dev(np.full(s, SENT, f32)) for k, s in shapes.items()}
    o["idx"] = X.dev(np.full((B, P, M), ISENT, np.int32))
    o["cnt"] = X.dev(np.full(B, ISENT, np.int32))
    one = X.dev(np.ones(1, f32))
    L = lib
    assert L.mf_pose_epilogue_train_fwd(p(d["orot"]), p(d["otrn"]), p(d["ocnf"]), p(d["class_id"]), p(d["pts"]),
                                        p(d["origin"]), p(d["pitch"]), B, P, nf, p(o["rot"]), p(o["trans"]), p(o["conf"]),
                                        X.stream) == 0
    assert L.mf_transformation_matrix_fwd(p(o["rot"]), p(o["trans"]), n, p(o["T_pred"]), X.stream) == 0
    assert L.mf_transformation_matrix_fwd(p(d["q_true"]), p(d["t_true"]), B, p(o["T_true"]), X.stream) == 0
    assert L.mf_average_distance_fwd(p(d["points"]), p(o["T_true"]), p(o["T_pred"]), p(d["sym"]), B, M, P, p(o["add"]),
                                     p(o["idx"]), X.stream) == 0
    assert L.mf_confidence_loss_fwd(p(o["add"]), p(o["conf"]), B, P, c["lam"], p(o["loss"]), p(o["cnt"]), X.stream) == 0
    assert L.mf_confidence_loss_bwd(p(o["add"]), p(o["conf"]), p(o["cnt"]), p(one), B, P, c["lam"], p(o["dadd"]),
                                    p(o["dconf"]), X.stream) == 0
    assert L.mf_average_distance_bwd(p(d["points"]), p(o["T_true"]), p(o["T_pred"]), p(d["sym"]), p(o["dadd"]), B, M, P,
                                     p(o["idx"]), p(o["gT"]), X.stream) == 0
    assert L.mf_transformation_matrix_bwd(p(o["rot"]), p(o["gT"]), n, p(o["gq"]), p(o["gt"]), X.stream) == 0
    assert L.mf_pose_epilogue_train_bwd(p(d["orot"]), p(d["ocnf"]), p(d["class_id"]), p(d["pitch"]), p(o["gq"]), p(o["gt"]),
                                        p(o["dconf"]), B, P, nf, p(o["drot"]), p(o["dtrn"]), p(o["dcnf"]), X.stream) == 0
    X.sync()
    return {k: X.host(v) for k, v in o.items()}


def chain_mirror_idx(c, T_true, T_pred):
    want = np.full((c["B"], c["P"], c["M"]), ISENT, np.int64)
    for b in range(c["B"]):
        if c["sym"][b]:
            pt = O.transform_points(c["points"][b], T_true[b])
            want[b] = O.nn(pt, O.transform_points(c["points"][b], T_pred[b]).reshape(-1, 3)).reshape(c["P"], c["M"])
    return want


def check_chain(c, got, tag):
    """STAGE BY STAGE: every kernel's output within that op's bound of the float64 reference evaluated on the
    float32 tensors the chain itself handed to that kernel (the propagated end-to-end bound would need every op's
    condition number; the per-op bounds on the chain's own intermediates pin the same arithmetic and the wiring).  The
    distance of the whole float32 chain from the whole float64 chain (arg-min frozen) is printed, not asserted."""
    g = {k: np.asarray(v) for k, v in got.items()}
    B, P, nf = c["B"], c["P"], c["nf"]
    n = B * P
    st = lambda s: f"{tag} chain {s}"  # noqa: E731
    ref, bnd = R.pose_epilogue(c["orot"], c["otrn"], c["ocnf"], c["class_id"], c["pts"], c["origin"], c["pitch"], nf)
    for k, r, b in zip(("rot", "trans", "conf"), ref, bnd):
        R.assert_within(g[k], r, b, st(k), op=f"{tag} chain")
    T, bT = R.transformation_matrix(g["rot"].reshape(n, 4), g["trans"].reshape(n, 3))
    R.assert_within(g["T_pred"].reshape(n, 4, 4), T, bT, st("T_pred"), op=f"{tag} chain")
    T, bT = R.transformation_matrix(c["q_true"], c["t_true"])
    R.assert_within(g["T_true"], T, bT, st("T_true"), op=f"{tag} chain")
    assert np.array_equal(g["idx"], chain_mirror_idx(c, g["T_true"], g["T_pred"])), st("arg-min rows vs the float32 mirror")
    args = (c["points"], g["T_true"], g["T_pred"], c["sym"])
    a, ba, _ = R.average_distance(*args, idx=g["idx"])
    R.assert_within(g["add"], a, ba, st("add"), op=f"{tag} chain")
    loss, bl, cnt = R.confidence_loss(g["add"], g["conf"], c["lam"])
    assert np.array_equal(g["cnt"], cnt)
    R.assert_within(g["loss"].reshape(()), np.asarray(loss), np.asarray(bl), st("loss"), op=f"{tag} chain")
    (dadd, dconf), (b1, b2) = R.confidence_loss_grad(g["add"], g["conf"], c["lam"], 1.0)
    R.assert_within(g["dadd"], dadd, b1, st("dadd"), op=f"{tag} chain")
    R.assert_within(g["dconf"], dconf, b2, st("dconf"), op=f"{tag} chain")
    gT, bg = R.average_distance_grad(*args, g["idx"], g["dadd"])
    R.assert_within(g["gT"], gT, bg, st("gT"), op=f"{tag} chain")
    (gq, gt), (bq, bt) = R.transformation_matrix_grad(g["rot"].reshape(n, 4), g["gT"].reshape(n, 4, 4))
    R.assert_within(g["gq"].reshape(n, 4), gq, bq, st("gq"), op=f"{tag} chain")
    R.assert_within(g["gt"].reshape(n, 3), gt, bt, st("gt"), op=f"{tag} chain")
    ref, bnd = R.pose_epilogue_grad(c["orot"], c["ocnf"], c["class_id"], c["pitch"], g["gq"], g["gt"], g["dconf"], nf)
    for k, r, b in zip(("drot", "dtrn", "dcnf"), ref, bnd):
        R.assert_within(g[k], r, b, st(k), op=f"{tag} chain")
    # the whole chain in float64, arg-min frozen to the (verified) indices: reported
    e = chain_f64(c, g["idx"])
    for k in ("loss", "drot", "dtrn", "dcnf"):
        scale = np.abs(e[k]).max()
        print(f"LOSSCHAIN {tag} chain end to end {k}: max |float32 chain - float64 chain| / max |.| = "
              f"{np.abs(g[k].reshape(e[k].shape) - e[k]).max() / scale:.3e}")
    assert np.isfinite(g["loss"]).all()


def chain_f64(c, idx):
    B, P, nf = c["B"], c["P"], c["nf"]
    n = B * P
    (rot, trans, conf), _ = R.pose_epilogue(c["orot"], c["otrn"], c["ocnf"], c["class_id"], c["pts"], c["origin"],
                                            c["pitch"], nf)
    Tp = R.transformation_matrix(rot.reshape(n, 4), trans.reshape(n, 3))[0].reshape(B, P, 4, 4)
    Tt = R.transformation_matrix(c["q_true"], c["t_true"])[0]
    args = (c["points"], Tt, Tp, c["sym"])
    add = R.average_distance(*args, idx=idx)[0]
    lam = float(np.float32(c["lam"]))
    loss = (add * conf - lam * np.log(conf)).mean(axis=1).mean()
    dadd, dconf = conf / (B * P), (add - lam / conf) / (B * P)
    gT = R.average_distance_grad(*args, idx, dadd)[0]
    (gq, gt), _ = R.transformation_matrix_grad(rot.reshape(n, 4), gT.reshape(n, 4, 4))
    (drot, dtrn, dcnf), _ = R.pose_epilogue_grad(c["orot"], c["ocnf"], c["class_id"], c["pitch"], gq, gt, dconf, nf)
    return dict(loss=np.asarray([loss]), drot=drot, dtrn=dtrn, dcnf=dcnf)


def report():
    for k in sorted(R.RATIOS):
        print(f"LOSSCHAIN worst error / bound, {k}: {R.RATIOS[k]:.3f}")
