"""TSDF colour without a GPU, on the mirror alone (tests/tsdfcolor_ref.py over tests/tsdfcolor_cases.py): the voxels that
take a colour are those that would vote; SAMPLE at a voxel centre, at the hand-placed points and where no corner is
coloured; what the fused colours mean (the mirror's colour image from a held-out pose against the analytic colour of the
same pixels); and what the sequences are there to show."""
import numpy as np
import pytest

import tsdfcolor_cases as C
import tsdfcolor_ref as CR
import tsdflabel_cases as LC
import tsdflabel_ref as LR

# mean absolute channel error (uint8 levels) measured on the mirror for sequence (a), 273 pixels (DESIGN.md "TSDF colour")
COLOR_FIDELITY = 1.376


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name)) for name in C.CASES}


def test_the_voxels_that_take_a_colour_are_those_that_would_vote():
    """Frame by frame over five frames and one with holes: colour weight rose exactly where tsdflabel_ref lets a voxel
    vote under a label image in which every pixel votes; every coloured voxel was written by the plain integrate."""
    vol, lab = CR.ColorVolume(**C.VOLUME), LR.InstanceVolume(**C.VOLUME)
    frames = [C.frame(k) for k in range(5)]
    frames[2][0][3:9, 4:12] = np.nan
    for depth, _, rgb, T in frames:
        before = vol.colors[..., 3].copy()
        what = vol.integrate(depth, C.K, T, color=rgb)
        vote = lab.integrate(depth, C.K, T, label=np.ones((C.H, C.W), np.int32))
        voted = np.isin(vote, (LR.CLAIM, LR.AGREE, LR.SATURATE))
        assert voted.sum() > 3000 and np.array_equal(vol.colors[..., 3] > before, voted)
        assert np.array_equal(np.isin(what, (CR.COLOURED, CR.SATURATED)), voted)
        assert np.array_equal(what == CR.FAR, vote == LR.FAR) and (what == CR.FAR).sum() > 1000
    assert np.array_equal(vol.volume, lab.volume)
    assert not ((vol.colors[..., 3] > 0) & ~(vol.volume[..., 1] > 0)).any()


def test_sampling_at_a_voxel_centre_returns_that_voxels_colour(mirror):
    """At the centre of a coloured voxel whose cell's corners are all coloured the weights are (1, 0, .., 0): the
    sample is the voxel's colour, rounded."""
    colors = mirror["a"][2]["colors"]
    has = colors[..., 3] > 0
    nz, ny, nx = has.shape
    full = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                full &= has[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    k, j, i = np.nonzero(full)
    assert k.size > 1000
    o, p = C.VOLUME["origin"], C.VOLUME["pitch"]
    idx = [i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)]
    m = [o[a] + p * idx[a] for a in range(3)]
    exact = np.all([(m[a] - o[a]) / p == idx[a] for a in range(3)], 0)  # the centres that land on their lattice point
    assert exact.sum() > 500
    got = CR.sample(colors, o, p, m)[exact]
    exp = np.floor(colors[k, j, i, :3].astype(np.float64) + 0.5).astype(np.uint8)[exact]
    assert (got[:, 3] == 255).all() and np.array_equal(got[:, :3], exp)


def test_alpha_is_zero_exactly_where_no_corner_is_coloured(mirror):
    """Over the held-out render's points, the mesh vertices, the hand-placed points and a grid of points through the
    whole box and beyond it: alpha is 255 where the point is usable and its cell has a coloured corner, else 0 with
    r = g = b = 0.  (No point here sits on a lattice plane of a cell whose only coloured corners have weight 0.)"""
    a = mirror["a"]
    colors, o, p = a[2]["colors"], C.VOLUME["origin"], C.VOLUME["pitch"]
    grid = np.stack(np.meshgrid(*[np.linspace(o[n] - 0.05, o[n] + p * C.VOLUME["dims"][n] + 0.03, 23) for n in range(3)],
                                indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([a[4]["vertices"], C.hand_points()[0], grid])
    out, usable, n_coloured = CR.sample(colors, o, p, [pts[:, 0], pts[:, 1], pts[:, 2]], return_corners=True)
    some = usable & (n_coloured > 0)
    assert some.sum() > 4000 and (~usable).sum() > 1000 and (usable & (n_coloured == 0)).sum() > 1000
    assert np.array_equal(out[:, 3] == 255, some) and not out[~some].any()
    assert set(np.unique(out[:, 3])) == {0, 255}
    assert set(np.unique(n_coloured[usable])) == set(range(9))  # every number of coloured corners occurs


def test_the_hand_placed_points_are_what_their_names_say(mirror):
    colors, o, p = mirror["a"][2]["colors"], C.VOLUME["origin"], C.VOLUME["pitch"]
    pts, names = C.hand_points()
    out, usable, n_coloured = CR.sample(colors, o, p, [pts[:, 0], pts[:, 1], pts[:, 2]], return_corners=True)
    assert np.array_equal(out, mirror["a"][5]["sampled"])
    row = {name: (out[n].tolist(), bool(usable[n]), int(n_coloured[n])) for n, name in enumerate(names)}
    for name in ("outside", "below", "last plane", "nan"):
        assert row[name] == ([0, 0, 0, 0], False, 0), name
    assert (pts[2, 0] - o[0]) / p == C.VOLUME["dims"][0] - 1 and (pts[4, 0] - o[0]) / p == 0.0
    assert row["inside last cell"][1:] == (True, 8) and row["inside last cell"][0][3] == 255
    assert row["first plane"][1:] == (True, 8) and row["first plane"][0][3] == 255
    assert row["no corner"] == ([0, 0, 0, 0], True, 0)
    # one coloured corner: the renormalised sample is that corner's colour whatever its weight
    assert row["one corner"][1:] == (True, 1) and row["one corner"][0][3] == 255
    g = [(pts[6, a] - o[a]) / p for a in range(3)]
    b = [int(np.floor(x)) for x in g]
    corner = colors[b[2]:b[2] + 2, b[1]:b[1] + 2, b[0]:b[0] + 2].reshape(8, 4)
    (only,) = np.flatnonzero(corner[:, 3] > 0)
    assert np.abs(np.asarray(row["one corner"][0][:3]) - corner[only, :3].astype(np.float64)).max() <= 0.5 + 1e-9
    # the ground's ramp and sphere 1's tint arrive
    assert np.abs(np.asarray(row["ground"][0][:3]) - (60.0 + 150.0 * 0.413, 80.0 + 160.0 * 0.129, 40.0)).max() < 4
    assert row["sphere 1"][0][0] > 190 and row["sphere 1"][0][2] < 70


def test_fused_colours_agree_with_the_analytic_colour(mirror):
    """Sequence (a) fused into the mirror, ray-cast from a held-out pose, colour_image against the analytic colour of
    the same pixels.  Condition: at least 0.9 of the pixels with depth have alpha 255.  Fidelity: the mean absolute
    channel error over the pixels with depth and alpha 255 stays below 1.5 times the value recorded from this mirror
    (the margin for the mirror's own later edits); the large errors sit on the spheres' silhouettes, where a 2 cm
    voxel holds both sides."""
    depth, image = mirror["a"][3]["depth"], mirror["a"][3]["color_image"]
    exp = C.analytic_color(*LC.render(C.HELD_OUT), C.HELD_OUT)
    has = depth > 0
    ok = has & (image[..., 3] == 255)
    coverage = ok.sum() / has.sum()
    error = np.abs(image[..., :3].astype(np.float64) - exp.astype(np.float64))[ok]
    print(f"alpha 255 on {int(ok.sum())} of {int(has.sum())} pixels with depth; mean |error| {error.mean():.4f}, "
          f"max {error.max():.0f}")
    assert has.sum() > 250 and coverage >= 0.9
    assert error.mean() < 1.5 * COLOR_FIDELITY
    assert not image[~has].any()  # a pixel without depth is (0, 0, 0, 0)
    labels = LC.render(C.HELD_OUT)[1]
    assert set(np.unique(labels[ok])) == {-1, 1, 3}  # the ramp and both tints are in the view


def test_what_the_cases_show(mirror):
    """The properties the sequences are there for, read off the mirror's results."""
    a, b, c, d, e = (mirror[name] for name in C.CASES)
    whats = set(np.unique(np.concatenate([r["what"].ravel() for res in mirror.values() for r in res if "what" in r])))
    assert whats == {-1, CR.NOT_UPDATED, CR.FAR, CR.COLOURED, CR.SATURATED}
    assert a[0]["colors"][..., 3].max() == 1 and a[2]["colors"][..., 3].max() == 3
    assert (a[2]["colors"][..., 3] > 0).sum() > 5000
    assert a[2]["colors"][..., :3].max() <= 255 and a[2]["colors"][..., :3].min() >= 0
    assert len(a[4]["vertices"]) > 3000 and (a[4]["vertex_colors"][:, 3] == 255).mean() > 0.9
    assert b[3]["colors"][..., 3].max() == 2 and b[3]["volume"][..., 1].max() == 2  # saturated at max_weight = 2
    assert b[3]["colors"].tobytes() != b[2]["colors"].tobytes()  # ... and the average still moves
    assert c[1]["colors"].tobytes() == c[0]["colors"].tobytes() and c[1]["volume"].tobytes() == c[0]["volume"].tobytes()
    assert c[3]["colors"].tobytes() != c[1]["colors"].tobytes()
    assert c[2]["color_image"][..., 3].any()
    away = c[4]["depth"] > 0  # from inside the box, looking up: a few rays meet a sphere from below, most meet nothing
    assert 0 < away.sum() < 50 and not c[4]["color_image"][~away].any()
    for n in (1, 3):  # color=None: the tsdf moves, the colours do not
        assert d[n]["colors"].tobytes() == d[n - 1]["colors"].tobytes()
        assert d[n]["volume"].tobytes() != d[n - 1]["volume"].tobytes()
    assert e[2]["colors"].tobytes() == e[1]["colors"].tobytes() and e[2]["labels"].tobytes() != e[1]["labels"].tobytes()
    assert e[3]["colors"].tobytes() != e[2]["colors"].tobytes() and e[3]["labels"].tobytes() == e[2]["labels"].tobytes()
    assert all(e[4][key].tobytes() == e[3][key].tobytes() for key in ("volume", "labels", "colors"))  # the skip word
