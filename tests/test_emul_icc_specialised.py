"""The specialised forms of the ICC iteration kernels (k_icc_fused3<MAXNS>) WITHOUT a GPU:
the kernel source on the fiber emulator with guard pages behind every array it is handed, and the plan that picks a
form as host arithmetic.  Cases and checks: tests/icc_specialised_ref.py (shared with the MI355X test)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import icc_cases as C
import icc_specialised_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul"))
import emul  # noqa: E402

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def lib():
    return emul.build(["icc.hip"])


def run_emul(lib, name, form):
    c = R.CASES[name]
    scenes, q0, t0 = R.make_case(name)
    with R.knob_env(c["cap"], form):
        S = emul.EmulIccScenes(lib, scenes, voxel_dim=c["dim"], voxel_threshold=c["thr"], sdf_offset=0.02)
        # every array the kernels are handed ends at an unmapped page: the batch, the workspace, the state, the outputs
        for field in ("pts4", "obj_off", "scene_off", "obj_scene", "pitch", "origin", "grid_target", "grid_ne"):
            g = emul.guarded(getattr(S, field))
            setattr(S, field, g)
            setattr(S.desc, field, g.ctypes.data)
        S.ws = emul.guarded(np.zeros(lib.mf_icc_workspace_bytes(ctypes.byref(S.desc)), np.uint8))
        S.ws_ptr = S.ws.ctypes.data
        assert S.ws_ptr % 256 == 0
        assert lib.mf_icc_prepare(ctypes.byref(S.desc), S.ws_ptr, None) == 0
        O, ns, n_iter = len(q0), len(scenes), R.N_ITER
        arrays = [emul.guarded(x) for x in (q0, t0, np.zeros((O, 7), np.float32), np.zeros((O, 7), np.float32),
                                            np.zeros((n_iter, ns), np.float32), np.zeros((n_iter, O, 7), np.float32))]
        S.refine(*arrays[:4], n_iter, losses=arrays[4], traj=arrays[5])
        out = {k: np.array(x) for k, x in zip(R.KEYS, arrays)}
        out["form"] = R.form_of(lib, S.desc)
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_specialised_forms_give_the_fall_backs_bits_and_the_oracles_steps(lib, name):
    auto = run_emul(lib, name, None)
    assert auto["form"] == R.CASES[name]["form"], auto["form"]
    generic = run_emul(lib, name, "generic")
    assert generic["form"] == R.GENERIC
    R.check_bitwise(auto, generic, "auto against MF_ICC_FUSED_FORM=generic")      # (i)
    R.check_vs_oracle(name, auto)                                                # (ii)
    R.check_bitwise(auto, run_emul(lib, name, "auto"), "two runs of auto")       # (iii)


def test_plan_picks_a_form_by_host_arithmetic_alone(lib, monkeypatch):
    """Every row of the eligibility table (csrc/icc.hip, at kFormGeneric), on descriptors of null pointers: nothing is
    launched, no device is touched.  A specialised form hard-codes kernel size 3, so it needs the proof that EVERY
    grid's ceil((thr * pitch) / pitch), made odd, is 3 whatever its pitch: thresholds whose float32 neighbourhood
    reaches 1 (size 1) or exceeds 3 (size 5) stay on the kernels that read the size per grid."""
    for k in ("MF_ICC_GENERAL", "MF_ICC_BIN_CAP", "MF_ICC_FUSED_FORM", "MF_ICC_DEBUG", "MF_ICC_LDS_PAD"):
        monkeypatch.delenv(k, raising=False)
    f = lambda *a, **k: R.form_of(lib, C.desc(*a, **k))   # noqa: E731
    assert f(8, 1, 8, n_points=28000, dim=32) == R.NS16             # the bench's scene
    assert f(64, 8, 8, n_points=8 * 28000, dim=32) == R.NS16        # value_scenes8
    assert f(8, 1, 8, n_points=0) == R.NS16 and f(5, 2, 3) == R.NS16                 # no points; ragged scenes
    assert f(16, 1, 16) == R.NS16 and f(17, 1, 17) == R.NS64
    assert f(64, 1, 64) == R.NS64 and f(65, 1, 65) == R.GENERIC                      # k_icc_fused_big stays what it is
    assert f(128, 1, 128) == R.GENERIC and f(129, 1, 129) == -1                      # 129 objects: refused as before
    assert C.query(lib, C.desc(129, 1, 129)) is None and C.query(lib, C.desc(128, 1, 128))["launches"] == 2
    # the threshold: 3 cells proved only strictly between 1 and 3, with the 2 ulp of the float32 quotient to spare
    up, down = (lambda x: float(np.nextafter(np.float32(x), np.float32(9)))), (lambda x: float(np.nextafter(np.float32(x), np.float32(0))))
    for thr, want in ((0.5, R.GENERIC), (down(1.0), R.GENERIC), (1.0, R.GENERIC), (up(1.0), R.GENERIC),
                      (up(up(up(1.0))), R.GENERIC), (1.00001, R.NS16), (1.5, R.NS16), (2.0, R.NS16), (2.9999, R.NS16),
                      (down(3.0), R.GENERIC), (3.0, R.GENERIC), (up(3.0), R.GENERIC), (4.0, R.GENERIC), (6.0, R.GENERIC)):
        assert f(8, 1, 8, thr=thr) == want, thr
    assert f(8, 1, 8, thr=7.0) == -1
    assert f(8, 1, 8, ne_binary=0) == R.GENERIC and f(8, 1, 8, dim=33) == R.GENERIC   # the two-kernel path
    assert C.query(lib, C.desc(8, 1, 8)) == C.plan(C.desc(8, 1, 8))                   # mf_icc_plan is what it was
    monkeypatch.setenv("MF_ICC_BIN_CAP", "3")
    assert f(8, 1, 8) == R.NS16                                                       # overflow records: every form reads them
    monkeypatch.delenv("MF_ICC_BIN_CAP")
    monkeypatch.setenv("MF_ICC_GENERAL", "1")
    assert f(8, 1, 8) == R.GENERIC
    monkeypatch.delenv("MF_ICC_GENERAL")
    monkeypatch.setenv("MF_ICC_FUSED_FORM", "generic")
    assert f(8, 1, 8) == R.GENERIC and f(17, 1, 17) == R.GENERIC
    assert C.query(lib, C.desc(8, 1, 8)) == C.plan(C.desc(8, 1, 8))
    monkeypatch.setenv("MF_ICC_FUSED_FORM", "auto")
    assert f(8, 1, 8) == R.NS16
