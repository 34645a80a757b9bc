"""The launch plan of csrc/icc.hip (icc_plan) without a GPU: the host-emulated build answers ``mf_icc_plan`` with the
very function the launchers, ``mf_icc_workspace_bytes`` and ``mf_icc_iteration_launches`` use, and every slot of every
answer is held against the rules restated in tests/icc_cases.py.  The grid has both neighbours of every threshold:
ceil(D / 2) * D <= 512 (D = 32 | 33), 64 | 65 objects per scene (k_icc_fused | k_icc_fused_big; the two-kernel path
valid | refused) and 128 | 129, 31 | 32 objects (xcd_order), kernel size 7 | 9 (threshold 6 | 7), point counts around a
multiple of the binning chunk, scenes of one size and not (uniform_ns), under every setting of MF_ICC_GENERAL and
MF_ICC_BIN_CAP.  Arithmetic on descriptors of null pointers: nothing is launched.  Also here: MF_ICC_DEBUG and
MF_ICC_LDS_PAD reach only a build with -DMF_ICC_DEBUG_BUILD=1."""
import ctypes
import itertools

import pytest

import icc_cases as C
from host_emul import emul

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")

KNOBS = ("MF_ICC_GENERAL", "MF_ICC_BIN_CAP", "MF_ICC_DEBUG", "MF_ICC_LDS_PAD")
SETTINGS = list(itertools.product((None, "0", "1"), (None, "3")))       # (MF_ICC_GENERAL, MF_ICC_BIN_CAP)

DIMS = (16, 31, 32, 33, 64, 65)
# (n_objects, n_scenes, max_scene_objects): one scene of N; a scene of N beside a scene of one object (not uniform
# from N = 2 on); 31 | 32 scenes of one object
OBJECTS = ([(N, 1, N) for N in (1, 32, 33, 64, 65, 128, 129)] + [(N + 1, 2, N) for N in (1, 32, 33, 64, 65, 128, 129)] +
           [(31, 31, 1), (32, 32, 1)])
POINTS = (0, 1, 1023, 1024, 1025, 28000)
THRESHOLDS = (2, 3, 6, 7)


def points():
    for dim, (O, S, N), P, thr, ne in itertools.product(DIMS, OBJECTS, POINTS, THRESHOLDS, (0, 1)):
        yield C.desc(O, S, N, n_points=P, dim=dim, thr=thr, ne_binary=ne)


@pytest.fixture(scope="module")
def L():
    return emul.build(["icc.hip"])


def set_knobs(monkeypatch, setting):
    for name, value in zip(KNOBS, tuple(setting) + (None,) * (len(KNOBS) - len(setting))):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def test_plan_equals_the_restated_rules_on_both_sides_of_every_threshold(L, monkeypatch):
    pts = list(points())
    seen = {}
    for general, cap in SETTINGS:
        set_knobs(monkeypatch, (general, cap))
        for d in pts:
            want, got = C.plan(d, general=general, bin_cap=cap), C.query(L, d)
            what = (d.n_objects, d.n_scenes, d.max_scene_objects, d.n_points, d.dim, d.voxel_threshold, d.grid_ne_binary,
                    general, cap)
            assert got == want, what
            # ... and the two older questions are answered by the same plan
            assert L.mf_icc_workspace_bytes(ctypes.byref(d)) == (want["ws_bytes"] if want else -1), what
            assert L.mf_icc_iteration_launches(ctypes.byref(d)) == (want["launches"] if want else -1), what
            key = "refused" if want is None else ("variant", want["variant"])
            seen[key] = seen.get(key, 0) + 1
            if want:
                for k in ("xcd_order", "uniform_ns"):
                    seen[(k, bool(want[k]))] = seen.get((k, bool(want[k])), 0) + 1
    # the grid did not shrink to nothing, and every outcome is in it many times
    assert len(pts) == len(DIMS) * 16 * len(POINTS) * len(THRESHOLDS) * 2 == 4608 and len(SETTINGS) == 6
    assert all(seen.get(k, 0) >= 500 for k in ("refused", ("variant", 0), ("variant", 1), ("variant", 2), ("xcd_order", False),
                                               ("xcd_order", True), ("uniform_ns", False), ("uniform_ns", True))), seen


def test_each_threshold_moves_the_slot_it_should(L, monkeypatch):
    """The neighbours of every threshold, one pair each, spelled out (the grid above has them among thousands)."""
    set_knobs(monkeypatch, ())
    q = lambda *a, **k: C.query(L, C.desc(*a, **k))   # noqa: E731
    assert q(8, 1, 8, dim=32)["single_pass"] == 1 and q(8, 1, 8, dim=33)["single_pass"] == 0
    assert q(64, 1, 64)["variant"] == C.FUSED and q(65, 1, 65)["variant"] == C.FUSED_BIG
    assert q(64, 1, 64, ne_binary=0)["variant"] == C.TILE_ACCUM and q(65, 1, 65, ne_binary=0) is None
    assert q(128, 1, 128)["launches"] == 2 and q(129, 1, 129) is None
    assert q(31, 31, 1)["xcd_order"] == 0 and q(32, 32, 1)["xcd_order"] == 1
    assert q(8, 1, 8, thr=6)["hmax"] == 3 and q(8, 1, 8, thr=7) is None
    assert q(8, 1, 8, n_points=1025)["n_tab"] - q(8, 1, 8, n_points=1024)["n_tab"] == 8    # 8 x 1025 points: a 9th chunk -> + 8
    assert q(8, 1, 8, n_points=1024)["n_tab"] == q(8, 1, 8, n_points=1023)["n_tab"]
    assert q(16, 2, 8)["uniform_ns"] == 8 and q(15, 2, 8)["uniform_ns"] == 0
    monkeypatch.setenv("MF_ICC_GENERAL", "1")
    assert q(8, 1, 8)["launches"] == 3 and q(65, 1, 65) is None
    monkeypatch.setenv("MF_ICC_GENERAL", "0")            # the code's rule: a number other than 0
    assert q(8, 1, 8)["launches"] == 2


def test_plan_query_refuses_malformed_questions(L, monkeypatch):
    set_knobs(monkeypatch, ())
    d = C.desc(8, 1, 8)
    out = (ctypes.c_int64 * len(C.SLOTS))()
    assert L.mf_icc_plan(ctypes.byref(d), out, len(C.SLOTS)) == len(C.SLOTS)
    assert L.mf_icc_plan(None, out, len(C.SLOTS)) < 0
    assert L.mf_icc_plan(ctypes.byref(d), None, len(C.SLOTS)) < 0
    assert L.mf_icc_plan(ctypes.byref(d), out, 0) < 0 and L.mf_icc_plan(ctypes.byref(d), out, -1) < 0
    assert L.mf_icc_plan(ctypes.byref(C.desc(8, 1, 8, flags=1)), out, len(C.SLOTS)) < 0
    assert C.query(L, d, n=3) == dict(single_pass=1, launches=2, variant=C.FUSED)     # (slots past n stay untouched)
    assert C.query(L, d, n=len(C.SLOTS)) == C.plan(d)


CASES_DBG = [C.desc(32, 32, 1), C.desc(31, 31, 1), C.desc(8, 1, 8), C.desc(96, 1, 96), C.desc(8, 1, 8, ne_binary=0)]


def test_debug_knobs_in_the_environment_do_not_reach_a_default_build(L, monkeypatch):
    """MF_ICC_DEBUG bit 4096 would switch xcd_order off at 32 objects, MF_ICC_LDS_PAD would grow the fused kernel's
    LDS: a default build answers exactly as with neither set."""
    set_knobs(monkeypatch, ())
    plain = [C.query(L, d) for d in CASES_DBG]
    set_knobs(monkeypatch, (None, None, "4096", "65536"))
    assert [C.query(L, d) for d in CASES_DBG] == plain == [C.plan(d) for d in CASES_DBG]
    assert plain[0]["xcd_order"] == 1
    set_knobs(monkeypatch, (None, None, "2048", None))
    assert [C.query(L, d) for d in CASES_DBG] == plain and plain[1]["xcd_order"] == 0


def test_debug_knobs_reach_a_debug_build(monkeypatch):
    Ld = emul.build(["icc.hip"], extra_flags=["-DMF_ICC_DEBUG_BUILD=1"])
    set_knobs(monkeypatch, ())
    plain = [C.query(Ld, d) for d in CASES_DBG]
    assert plain == [C.plan(d) for d in CASES_DBG] and plain[0]["xcd_order"] == 1
    set_knobs(monkeypatch, (None, None, "4096", "65536"))      # read again on every call
    for d, p0 in zip(CASES_DBG, plain):
        got = C.query(Ld, d)
        assert got == C.plan(d, dbg=4096, lds_pad=65536)
        assert got["xcd_order"] == 0
        assert got["lds_fused"] == (p0["lds_fused"] + 65536 if p0["single_pass"] else 0)   # whichever fused kernel runs
    set_knobs(monkeypatch, (None, None, "2048", None))
    assert C.query(Ld, CASES_DBG[1])["xcd_order"] == 1 and C.query(Ld, CASES_DBG[1]) == C.plan(CASES_DBG[1], dbg=2048)
