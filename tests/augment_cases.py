"""TEST INFRASTRUCTURE: the augmentation checks shared by tests/test_emul_augment.py (host emulator, 64 x 64) and
tests/test_gpu_augment.py (MI355X, 256 x 256, n = 16).  Every check takes the device string and the image size;
cases and bounds are the same on both."""
import colorsys

import numpy as np
import scipy.ndimage
import torch

import augment_ref as R
import render_cases as C
import morefusion_amd as mf
from morefusion_amd.datasets import augmentation as A


def crops(dev, S, n):
    """rgb u8 [n, S, S, 3], pcd f64 [n, S, S, 3] of make_cad_frame objects through instance_crops."""
    H, W = (480, 640) if dev != "cpu" else (120, 160)
    meshes = {c: C.ycb(c) for c in C.YCB}
    rgbs, pcds, seed = [], [], 0
    while sum(len(r) for r in rgbs) < n:
        f = mf.synthetic.make_cad_frame(meshes, seed=seed, height=H, width=W, n_objects=3, device=dev)
        t = lambda x: torch.as_tensor(x).to(dev)  # noqa: E731
        out = mf.geometry.instance_crops(t(f["rgb"]), t(f["depth"]).float(), f["K"], t(f["label"]).int(),
                                         np.asarray(f["instance_ids"], np.int32), image_size=S, min_valid=1)
        keep = out["keep"].cpu().numpy()
        rgbs.append(out["rgb"].cpu().numpy()[keep])
        pcds.append(out["pcd"].cpu().numpy()[keep].astype(np.float64))
        seed += 1
    return np.concatenate(rgbs)[:n], np.concatenate(pcds)[:n]


def from_masks(masks, seed=0, dtype=np.float64):
    """Random colours and coordinates below 4 m, NaN outside each mask."""
    rs = np.random.RandomState(seed)
    n, S = len(masks), masks[0].shape[0]
    rgb = rs.randint(0, 256, (n, S, S, 3)).astype(np.uint8)
    pcd = rs.uniform(0.3, 1.5, (n, S, S, 3)).astype(dtype)
    pcd[~np.stack(masks)] = np.nan
    return rgb, pcd


def blobs10(S):
    m = np.zeros((S, S), bool)
    b = S // 8
    for k in range(10):
        y, x = (k // 5) * 3 * b + b, (k % 5) * (S // 5) + 2
        m[y:y + b + k, x:x + b // 2 + 1] = True  # sizes all different: blob 9 is the largest
    return m


def hand_masks(S):
    yy, xx = np.mgrid[:S, :S]
    empty, full = np.zeros((S, S), bool), np.ones((S, S), bool)
    single = empty.copy()
    single[S // 3, S // 2] = True
    spiral = empty.copy()  # a one-pixel wide rectangular spiral, one blank pixel between its arms: one component
    y, x, dy, dx = 0, 0, 0, 1
    spiral[0, 0] = True
    inside = lambda a, b: 0 <= a < S and 0 <= b < S  # noqa: E731
    while True:
        for _ in range(2):  # straight on, else one clockwise turn
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not spiral[ny, nx] and not (inside(ay, ax) and spiral[ay, ax]):
                y, x = ny, nx
                spiral[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            break
    assert scipy.ndimage.label(spiral, structure=np.ones((3, 3)))[1] == 1 and spiral.sum() > S * S // 3
    checker = ((yy + xx) % 2 == 0)  # diagonal checkerboard: one 8-connected component
    checker[:, 0] = checker[:, -1] = checker[0] = checker[-1] = True
    checker[:, 1] = checker[:, -2] = checker[1] = checker[-2] = True  # two pixels wide at the borders
    lattice = (yy % 2 == 0) & (xx % 2 == 0)  # isolated pixels: (S / 2)^2 components
    two = empty.copy()
    two[S // 8:S // 4, S // 8:S // 2] = True
    two[S // 2:S // 2 + S // 8, S // 4:S // 4 + 3 * S // 8] = True  # equal sizes: the tie goes to the lower id
    assert two[:S // 2].sum() == two[S // 2:].sum()
    top = empty.copy()
    top[:S // 8] = True  # with case 0 and u = 8 the cut removes everything
    ring = empty.copy()  # largest component spans the image: identity re-centring
    ring[0] = ring[-1] = ring[:, 0] = ring[:, -1] = True
    ring[S // 4:S // 4 + 4, S // 4:S // 2] = True
    ring[S // 2 + 3:S // 2 + 6, S // 3:S // 2 + 5] = True
    return dict(empty=empty, full=full, single=single, spiral=spiral, checker=checker, lattice=lattice, two=two,
                top=top, ring=ring, blobs=blobs10(S))


def case_params(n, seed, names=()):
    """Drawn rows with the cut cases 0-3 in turn, the minimum and the no-op resize, a skipped blur; the `top` mask's
    row gets u = 8 (outside the drawn range: the only way a cut can remove a whole mask)."""
    p = A.draw_params(n, np.random.RandomState(seed))
    p[:, A.P_CUT_CASE] = np.arange(n) % 4
    p[0 % n, A.P_SCALE], p[1 % n, A.P_SCALE], p[2 % n, A.P_SIGMA] = 0.25, 0.999, 5e-4
    for k, name in enumerate(names):
        if name == "top":
            p[k, A.P_CUT_CASE], p[k, A.P_CUT_U] = 0, 8.0
        if name == "ring":
            p[k, A.P_CUT_U], p[k, A.P_BLOB_U] = 0.0, 0.0
    return p


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run_mask(dev, rgb, pcd, params, seed, **kw):
    out = A.augment_mask(_t(rgb, dev), _t(pcd, dev), params, seed, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_float(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def check_bitwise(dev, S, n):
    """Mask stage, colour stage and drop-out pattern equal the mirror; noised coordinates within 2^-21 m."""
    hm = hand_masks(S)
    names = list(hm)
    rgb_h, pcd_h = from_masks([hm[k] for k in names], seed=1)
    rgb_c, pcd_c = crops(dev, S, n)
    worst = 0.0
    for rgb, pcd, nm, dtype in ((rgb_c, pcd_c, (), np.float64), (rgb_h, pcd_h, names, np.float32)):
        pcd = pcd.astype(dtype)
        for seed in (3, 4):
            params = case_params(len(rgb), seed, nm)
            got = run_mask(dev, rgb, pcd, params, seed, return_components=True)
            ref = [R.augment_mask(rgb[i], pcd[i], params[i], seed) for i in range(len(rgb))]
            for k in ("keep", "kept_mask", "stats", "rgb", "labels", "sizes"):
                want = np.stack([r[k] for r in ref])
                assert np.array_equal(got[k], want), (k, nm, np.argwhere(got[k] != want)[:5])
            want_pcd = np.stack([r["pcd"] for r in ref])
            assert got["pcd"].dtype == dtype and _same_float(got["pcd"], want_pcd)
            for i, name in enumerate(nm):
                assert got["keep"][i] == (name not in ("empty", "top")), name
            out_rgb = A.augment_rgb(_t(got["rgb"], dev), params).cpu().numpy()
            want = np.stack([R.augment_rgb(got["rgb"][i], params[i]) for i in range(len(rgb))])
            assert np.array_equal(out_rgb, want), np.argwhere(out_rgb != want)[:5]
            out_pcd = A.augment_pcd(_t(got["pcd"], dev), params, seed).cpu().numpy()
            for i in range(len(rgb)):
                want_p, drop = R.augment_pcd(got["pcd"][i], params[i], seed)
                valid = ~np.isnan(got["pcd"][i]).any(-1)
                assert np.array_equal(np.isnan(out_pcd[i]), np.isnan(want_p))
                assert np.array_equal(valid & np.isnan(out_pcd[i]).any(-1), valid & drop)  # the drop-out pattern
                live = ~np.isnan(want_p)
                if live.any():
                    assert np.abs(want_p[live]).max() < 4.0
                    worst = max(worst, float(np.abs(out_pcd[i][live] - want_p[live]).max()))
    print(f"augment {S}x{S}: worst |noised coordinate - mirror| = {worst:.3e} (bound {2.0 ** -21:.3e})")
    assert worst <= 2.0 ** -21
    return worst


def check_determinism_and_batch_independence(dev, S, n):
    rgb, pcd = crops(dev, S, n)
    a = [x.cpu().numpy() for x in mf.datasets.augment_rgbd(_t(rgb, dev), _t(pcd, dev), random_state=7)]
    b = [x.cpu().numpy() for x in mf.datasets.augment_rgbd(_t(rgb, dev), _t(pcd, dev), np.random.RandomState(7))]
    assert np.array_equal(a[0], b[0]) and _same_float(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[1].dtype == np.float64 and a[2].all()
    rs = np.random.RandomState(7)
    params = A.draw_params(n, rs)
    seed = int(rs.randint(0, 2 ** 32, dtype=np.int64))
    ref = R.augment_rgbd(rgb, pcd, params, seed)  # the documented drawing order: table, then seed
    assert np.array_equal(a[0], ref[0]) and np.array_equal(np.isnan(a[1]), np.isnan(ref[1]))
    for sub in ([n - 1], [2, 0], list(range(n))[::-1]):
        m = run_mask(dev, rgb[sub], pcd[sub], params[sub], seed)
        c = A.augment_rgb(_t(m["rgb"], dev), params[sub]).cpu().numpy()
        p = A.augment_pcd(_t(m["pcd"], dev), params[sub], seed).cpu().numpy()
        assert np.array_equal(c, a[0][sub]) and _same_float(p, a[1][sub])
    before = (rgb.copy(), pcd.copy())
    r_t, p_t = _t(rgb, dev), _t(pcd, dev)
    mf.datasets.augment_rgbd(r_t, p_t, 1)
    assert np.array_equal(r_t.cpu().numpy(), before[0]) and _same_float(p_t.cpu().numpy(), before[1])


def check_components(dev, S, n):
    """Labels against scipy.ndimage.label (8-connectivity) up to renaming, sizes equal, the largest always kept."""
    hm = hand_masks(S)
    names = list(hm)
    rgb_h, pcd_h = from_masks([hm[k] for k in names], seed=2)
    rgb_c, pcd_c = crops(dev, S, n)
    rgb, pcd = np.concatenate([rgb_h, rgb_c]), np.concatenate([pcd_h, pcd_c])
    params = case_params(len(rgb), 5, names)
    got = run_mask(dev, rgb, pcd, params, 11, return_components=True)
    for i in range(len(rgb)):
        lab, size = got["labels"][i], got["sizes"][i]
        mask = lab >= 0
        ref, m = scipy.ndimage.label(mask, structure=np.ones((3, 3)))
        if not mask.any():
            assert not got["keep"][i]
            continue
        assert got["stats"][i, 4] == m
        pairs = np.unique(np.stack([lab[mask], ref[mask]], 1), axis=0)
        assert len(pairs) == m and len(np.unique(pairs[:, 0])) == m and len(np.unique(pairs[:, 1])) == m
        counts = np.bincount(ref.ravel())
        assert np.array_equal(size[mask], counts[ref[mask]])
        first = scipy.ndimage.minimum(np.arange(S * S).reshape(S, S), ref, np.arange(1, m + 1))
        assert np.array_equal(lab[mask], first[ref[mask] - 1])  # canonical id: first pixel in raster order
        big = size == size.max()
        lowest = lab[big].min()
        assert got["stats"][i, 6] == lowest and got["kept_mask"][i][lab == lowest].all()
        assert not (got["kept_mask"][i] & ~mask).any()
    k = names.index("lattice")
    assert got["stats"][k, 4] >= (S // 2 - 1) ** 2 // 2  # thousands of components: no cap
    k = names.index("two")
    assert got["stats"][k, 6] == got["labels"][k][got["labels"][k] >= 0].min()  # tie: the lower id


def check_blob_count_distribution(dev, S):
    """K = floor(u m) over 200 seeds on a 10-blob mask takes every value in 0..9.  Each value has probability 0.1
    per seed, so a given value is missed with probability 0.9^200 = 7.1e-10 and any of the ten with probability
    below 10 * 0.9^200 = 7.1e-9 (union bound): the assertion cannot fail by chance in practice.  Also: the kept
    components are exactly the largest plus the K smallest words."""
    n = 200
    rgb, pcd = from_masks([blobs10(S)] * n, seed=3)
    params = np.concatenate([A.draw_params(1, np.random.RandomState(s)) for s in range(n)])
    params[:, A.P_CUT_U] = 0.0
    got = run_mask(dev, rgb, pcd, params, 5, return_components=True)
    assert (got["stats"][:, 4] == 10).all()
    K = got["stats"][:, 5]
    assert sorted(set(K.tolist())) == list(range(10)), np.bincount(K, minlength=10)
    for i in range(n):
        ids = np.unique(got["labels"][i][got["labels"][i] >= 0])
        words = R.philox(5, params[i, A.P_KEY], ids, 0)[:, 0]
        want = set(ids[np.lexsort((ids, words))][:K[i]].tolist()) | {int(got["stats"][i, 6])}
        assert set(np.unique(got["labels"][i][got["kept_mask"][i]]).tolist()) == want


def check_hsv_round_trip(dev, S, n):
    """Neutral parameters, sigma below the skip threshold, scale 1: the colour stage is cv2's 8-bit RGB -> HSV ->
    RGB.  Bound per pixel against float64 colorsys (whose round trip is the identity up to 1e-12), with v the
    largest channel and d = max - min, in grey levels:
      V = v is exact, so the largest channel comes back exactly (v / 255 * 255 rounds to v): bound 0;
      S = rint-shift of d * rint(255 * 4096 / v) / 4096: the table entry is off by <= 0.5, so S is off by
        <= 0.5 + d * 0.5 / 4096 <= 0.532 units of 1/255; the smallest channel v (1 - s) moves by <= 0.532 v / 255
        <= 0.532 and the final rounding adds 0.5: |error| <= 1.032, an integer, so <= 1;
      H in 2-degree units, off by <= 0.5 + 6 d * 0.5 / 4096 <= 0.687 units = 0.0229 of a 60-degree sector; the
        middle channel v (1 - s f) moves by <= 0.532 (from S) + d * 0.0229 (from f, as v s = d) + 0.5 (rounding)
        + 0.01 (float32 arithmetic): <= floor(1.042 + 0.0229 d), at most 6 at d = 255."""
    rgb, _ = crops(dev, S, n)
    rs = np.random.RandomState(0)
    rgb = np.concatenate([rgb, rs.randint(0, 256, (2, S, S, 3)).astype(np.uint8)])
    params = A.neutral_params(len(rgb))
    params[:, A.P_SIGMA] = 5e-4
    out = A.augment_rgb(_t(rgb, dev), params).cpu().numpy().astype(np.int64)
    a = rgb.astype(np.int64)
    err = np.abs(out - a)
    order = np.argsort(a, axis=-1)
    e_sorted = np.take_along_axis(err, order, -1)
    d = a.max(-1) - a.min(-1)
    # where two channels tie the roles are shared: every channel then obeys the larger of its possible bounds
    mid_bound = np.floor(1.042 + 0.0229 * d).astype(np.int64)
    a_sorted = np.take_along_axis(a, order, -1)
    tie_hi, tie_lo = a_sorted[..., 1] == a_sorted[..., 2], a_sorted[..., 1] == a_sorted[..., 0]
    print(f"hsv round trip {S}x{S}: worst error min/mid/max channel = {e_sorted[..., 0].max()}, "
          f"{e_sorted[..., 1].max()}, {e_sorted[..., 2].max()}")
    assert (e_sorted[..., 2] <= np.where(tie_hi, mid_bound, 0)).all()
    assert (e_sorted[..., 1] <= mid_bound).all()
    assert (e_sorted[..., 0] <= np.where(tie_lo, mid_bound, 1)).all()
    pick = rs.randint(0, a[..., 0].size, 2000)
    for px, got in zip(a.reshape(-1, 3)[pick], out.reshape(-1, 3)[pick]):
        back = np.array(colorsys.hsv_to_rgb(*colorsys.rgb_to_hsv(*(px / 255.0)))) * 255.0
        assert np.abs(back - px).max() < 1e-9
        assert np.abs(got - back).max() <= np.floor(1.042 + 0.0229 * (px.max() - px.min())) + 1e-9


def check_blur(dev, S, n):
    """Colour-stage output blurred = scipy correlate1d with the mirror's weights (mode="mirror" = reflect-101) along
    both axes, within 1 level (the kernel rounds once, in integers)."""
    rgb, _ = crops(dev, S, n)
    params = A.neutral_params(len(rgb))
    params[:, A.P_SIGMA] = np.linspace(0.05, 1.0, len(rgb))
    out = A.augment_rgb(_t(rgb, dev), params).cpu().numpy()
    for i in range(len(rgb)):
        base = R.colour(rgb[i], 1, 1, 1, 1).astype(np.float64)
        w = R.blur_weights(params[i, A.P_SIGMA]) / 256.0
        want = scipy.ndimage.correlate1d(scipy.ndimage.correlate1d(base, w, axis=0, mode="mirror"), w, axis=1,
                                         mode="mirror")
        assert np.abs(out[i].astype(np.float64) - want).max() <= 1.0
    assert (out != rgb).any()


def _corr(a, b):
    return float(np.corrcoef(a.astype(np.float64), b.astype(np.float64))[0, 1])


def check_point_statistics(dev, S, n):
    """Drop-out fraction, noise mean and deviation, and independence between examples and between seeds: 5 sigma."""
    _, pcd = crops(dev, S, n)
    params = A.neutral_params(n)
    out = A.augment_pcd(_t(pcd, dev), params, 123).cpu().numpy()
    valid = ~np.isnan(pcd).any(-1)
    N = int(valid.sum())
    dropped = valid & np.isnan(out).any(-1)
    frac = dropped.sum() / N
    print(f"drop-out {frac:.5f} over {N} valid pixels")
    assert abs(frac - 0.05) <= 5 * np.sqrt(0.05 * 0.95 / N)
    noise = (out - pcd)[valid & ~dropped].ravel()
    M = noise.size
    print(f"noise mean {noise.mean():.3e}, std {noise.std(ddof=1):.6f} over {M}")
    assert abs(noise.std(ddof=1) - 0.003) <= 5 * 0.003 / np.sqrt(2 * M)
    assert abs(noise.mean()) <= 5 * 0.003 / np.sqrt(M)
    full = np.random.RandomState(0).uniform(0.3, 1.5, (2, S, S, 3))
    a = A.augment_pcd(_t(full, dev), params[:2], 123).cpu().numpy()
    b = A.augment_pcd(_t(full, dev), params[:2], 124).cpu().numpy()
    P = S * S
    for x, y, fx, fy in ((a[0], a[1], full[0], full[1]), (a[0], b[0], full[0], full[0])):  # two examples; two seeds
        dx, dy = np.isnan(x).any(-1).ravel(), np.isnan(y).any(-1).ravel()
        assert abs(_corr(dx, dy)) <= 5 / np.sqrt(P)
        both = ~dx & ~dy
        nx, ny = (x - fx).reshape(-1, 3)[both].ravel(), (y - fy).reshape(-1, 3)[both].ravel()
        assert abs(_corr(nx, ny)) <= 5 / np.sqrt(nx.size)


def check_reference_properties(dev, S, n):
    hm = hand_masks(S)
    names = list(hm)
    rgb_h, pcd_h = from_masks([hm[k] for k in names], seed=4)
    rgb_c, pcd_c = crops(dev, S, n)
    rgb, pcd = np.concatenate([rgb_h, rgb_c]), np.concatenate([pcd_h, pcd_c])
    params = case_params(len(rgb), 9, names)
    got = run_mask(dev, rgb, pcd, params, 21)
    for i in range(len(rgb)):
        valid_out = ~np.isnan(got["pcd"][i]).any(-1)
        if not got["keep"][i]:
            assert not valid_out.any() and not got["rgb"][i].any()
            continue
        # nearest sampling copies points: undoing the centring, every output point is a kept, valid input point
        src = {p.tobytes() for p in pcd[i][got["kept_mask"][i]]}
        assert all(p.tobytes() in src for p in got["pcd"][i][valid_out])
        assert not (got["kept_mask"][i] & np.isnan(pcd[i]).any(-1)).any()
        ys, xs = np.flatnonzero(valid_out.any(1)), np.flatnonzero(valid_out.any(0))
        y1, x1, y2, x2 = got["stats"][i, :4]
        if y2 - y1 >= x2 - x1:
            assert ys[0] == 0 and ys[-1] == S - 1
        if x2 - x1 >= y2 - y1:
            assert xs[0] == 0 and xs[-1] == S - 1
    k = names.index("ring")  # the kept component spans the image: the output is the masked input itself
    kept = got["kept_mask"][k]
    assert got["stats"][k, 5] == 0 and kept.sum() == 4 * S - 4
    assert not got["rgb"][k][~kept].any() and np.isnan(got["pcd"][k][~kept]).all()
    assert np.array_equal(got["rgb"][k][kept], rgb[k][kept]) and np.array_equal(got["pcd"][k][kept], pcd[k][kept])
