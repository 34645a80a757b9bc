"""The TSDF render's mirror (tests/tsdfrender_ref.py) against the mirrors it must agree with, no product code involved:
on every case of tests/tsdfrender_cases.py and B = 2, 4, 8 the skipping render gives the bytes of tsdf_ref's ray-cast
(depth, end code) and of tsdflabel_ref's label image of that depth -- which pins "FREE => F == 1" and "UNKNOWN =>
invalid" against the unskipped arithmetic -- and the cases exercise what they are there for (conditions on the inputs:
a failure here means the inputs must change, not the thresholds)."""
import numpy as np
import pytest

import tsdf_ref as R
import tsdflabel_ref as LR
import tsdfrender_cases as C
import tsdfrender_ref as RR


@pytest.fixture(scope="module")
def mirror():
    return {name: C.run_mirror(C.make_case(name), reference=True) for name in C.NAMES}


def _renders(mirror, names=C.NAMES, blocks=C.BLOCKS):
    return [(name, n, B, res[B]) for name in names for n, res in enumerate(mirror[name]) for B in blocks]


@pytest.mark.parametrize("name", C.NAMES)
def test_skipping_render_equals_the_raycast_and_the_label_image(mirror, name):
    assert mirror[name]
    for n, res in enumerate(mirror[name]):
        depth, code = res["raycast"]
        origin, pitch, K, T, min_count = res["args"]
        label = LR.label_image(res["labels"], origin, pitch, depth, K, T, min_count)
        for B in C.BLOCKS:
            got = res[B]
            assert got["depth"].dtype == np.float32 and got["code"].dtype == np.uint8 and got["label"].dtype == np.int32
            assert got["depth"].tobytes() == depth.tobytes(), (n, B)
            assert got["code"].tobytes() == code.tobytes(), (n, B)
            assert got["label"].tobytes() == label.tobytes(), (n, B)
            assert (got["sampled"] <= got["total"]).all() and (got["sampled"] >= 0).all()
    if name == "labels":  # the label check is about something: ids, the background and 0 all occur
        assert {-1, 0, 1, 3} <= set(np.unique(mirror[name][0][4]["label"]).tolist())


def test_all_three_block_codes_and_clipped_last_blocks(mirror):
    for B in C.BLOCKS:
        for name in ("deep", "labels"):
            summary = mirror[name][-1][B]["summary"]
            assert summary.shape == RR.summary_shape(C.make_case(name)["volume"]["dims"], B)
        if B < 8:  # (deep has no 32 cm of free space, labels no 16 cm of unseen space: two codes each for B = 8)
            assert set(np.unique(mirror["deep"][1][B]["summary"]).tolist()) == {RR.MIXED, RR.FREE, RR.UNKNOWN}, B
        assert any((n - 1) % B for n in C.DEEP_VOLUME["dims"]), B  # a clipped last block
    assert set(np.unique(mirror["labels"][0][4]["summary"]).tolist()) == {RR.MIXED, RR.FREE, RR.UNKNOWN}
    assert any((n - 1) % 8 for n in C.make_case("labels")["volume"]["dims"])
    assert set(np.unique(mirror["deep"][1][8]["summary"]).tolist()) == {RR.MIXED, RR.UNKNOWN}
    assert set(np.unique(mirror["labels"][0][8]["summary"]).tolist()) == {RR.MIXED, RR.FREE}
    # the clipped blocks are not all of one kind: the codes of the last layer along x differ
    assert len(np.unique(mirror["deep"][1][4]["summary"][:, :, -1])) > 1


def test_a_quarter_of_the_main_renders_samples_are_skipped(mirror):
    name, n = C.MAIN
    for B in C.BLOCKS:
        res = mirror[name][n][B]
        total, sampled = int(res["total"].sum()), int(res["sampled"].sum())
        print(f"B = {B}: {total} samples, {sampled} evaluated, {1 - sampled / total:.3f} skipped")
        assert total > 5000
        if B == 4:
            assert total - sampled >= total / 4
    assert (mirror[name][n][4]["code"] == R.HIT).sum() > 300


def test_the_rays_the_cases_are_there_for(mirror):
    every = _renders(mirror)
    # 1. a hit whose previous sample was in a FREE block (P = 1 exactly meets F <= 0): needs step > truncation
    assert any(((r["code"] == R.HIT) & (r["before"] == RR.FREE)).any() for *_, r in every)
    for name in ("deep", "labels"):
        assert any(((r["code"] == R.HIT) & (r["before"] == RR.FREE)).sum() >= 5 for *_, r in _renders(mirror, [name]))
    # 2. a back face right after an UNKNOWN run, from behind the plane
    assert (mirror["deep"][4][2]["code"] == R.BACKFACE).sum() > 300
    behind = [mirror["deep"][8][B] for B in C.BLOCKS]
    assert any(((r["code"] == R.BACKFACE) & (r["before"] == RR.UNKNOWN)).sum() > 100 for r in behind)
    # 3. LEFT while inside a FREE block and while inside an UNKNOWN block
    assert any(((r["code"] == R.LEFT) & (r["before"] == RR.FREE)).any() for r in mirror["deep"][1].values()
               if isinstance(r, dict))
    assert any(((r["code"] == R.LEFT) & (r["before"] == RR.UNKNOWN)).any() for r in mirror["deep"][0].values()
               if isinstance(r, dict))
    # 4. CAP with max_steps inside a FREE run (3 samples) and the cap at 9
    for B in C.BLOCKS:
        capped = mirror["deep"][6][B] if B < 8 else mirror["labels"][3][B]  # (deep has no FREE block of 32 cm)
        assert (capped["code"] == R.CAP).sum() > 500 and ((capped["code"] == R.CAP) & (capped["before"] == RR.FREE)).sum() > 100
        assert (capped["total"][capped["code"] == R.CAP] == (3 if B < 8 else 4)).all()
        assert (mirror["deep"][7][B]["code"] == R.CAP).any()
    # 5. all five end codes
    assert set().union(*(np.unique(r["code"]).tolist() for *_, r in every)) == {R.HIT, R.LEFT, R.BACKFACE, R.MISS, R.CAP}
    assert (mirror["deep"][5][4]["code"] == R.MISS).any()
    # 6. a fresh volume is all UNKNOWN, nothing is evaluated inside it
    for B in C.BLOCKS:
        fresh = mirror["deep"][0][B]
        assert (fresh["summary"] == RR.UNKNOWN).all() and set(np.unique(fresh["code"])) <= {R.LEFT, R.MISS}
        assert not fresh["depth"].any() and (fresh["code"] == R.LEFT).sum() > 300
    # 7. a volume whose every voxel was seen free: all FREE, every ray LEFT; the only samples that are not skipped are
    # those on the box's faces, whose floor(g) names no cell (at most the first and the last one)
    for B in C.BLOCKS:
        free = mirror["free"][0][B]
        assert (free["summary"] == RR.FREE).all() and (free["code"] == R.LEFT).all()
        assert (free["sampled"] <= 2).all() and (free["total"] >= 4).all() and (free["before"] != RR.UNKNOWN).all()


def test_an_unseen_one_and_a_seen_almost_one_make_their_blocks_mixed(mirror):
    """(tsdf 1, weight 0) next to seen voxels and (weight 1, the float32 below 1): every block whose footprint holds
    one of them is MIXED, every other block stays FREE, and rays that cross them are evaluated there."""
    ops = C.make_case("free")["ops"]
    pokes = [op for op in ops if op[0] == "poke"]
    assert pokes[0][2:] == (1.0, 0.0) and pokes[1][3] == 1.0 and np.float32(pokes[1][2]) < 1
    assert np.float32(pokes[1][2]) == np.nextafter(np.float32(1), np.float32(0))
    nz, ny, nx = C.FREE_VOLUME["dims"][::-1]
    for B in C.BLOCKS:
        summary = mirror["free"][1][B]["summary"]
        expected = np.full_like(summary, RR.FREE)
        for _, (k, j, i), _, _ in pokes:
            for K in range(summary.shape[0]):
                for J in range(summary.shape[1]):
                    for I in range(summary.shape[2]):
                        if all(B * b <= v <= min(B * b + B, n - 1) for b, v, n in ((K, k, nz), (J, j, ny), (I, i, nx))):
                            expected[K, J, I] = RR.MIXED
        assert np.array_equal(summary, expected) and (expected == RR.MIXED).any() and (expected == RR.FREE).any()
        assert mirror["free"][1][B]["sampled"].any()
    # a voxel on a shared layer (index 2 = a multiple of B = 2) is in the footprint of both neighbours
    assert (mirror["free"][1][2]["summary"] == RR.MIXED).sum() > 2


def test_nan_weights_are_unknown_and_nan_tsdf_is_not_free():
    vol = R.fresh((5, 5, 5))
    vol[..., 1] = np.nan
    assert (RR.block_summary(vol, 4) == RR.UNKNOWN).all()
    vol[..., 1] = 1.0
    assert (RR.block_summary(vol, 4) == RR.FREE).all()
    vol[2, 2, 2, 0] = np.nan
    assert (RR.block_summary(vol, 4) == RR.MIXED).all()
    assert RR.block_summary(R.fresh((18, 3, 2)), 16).shape == (1, 1, 2)
