"""mf_icc_refine_converge (refine until each scene's loss has converged, per scene, on the device) through the kernel
SOURCE on the CPU emulator (tests/host_emul), against the FIXED loop: tests/icc_converge_ref.py derives from the
existing ``refine`` where each scene must stop and the bits it must be frozen in.  tests/test_gpu_icc_converge.py
repeats this on the MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul"))
import emul  # noqa: E402

import icc_converge_ref as R  # noqa: E402

pytestmark = pytest.mark.skipif(not emul.available(), reason="g++ not available")


@pytest.fixture(scope="module")
def lib():
    return emul.build(["icc.hip"])


@pytest.fixture(scope="module", params=sorted(R.RAGGED_CASES))
def ragged(request, lib, fixtures3):
    """One ragged batch (scenes of 2, 3 and 1 objects) per iteration layout, with the fixed loop's answers shared by
    the tests below."""
    case = R.RAGGED_CASES[request.param]
    scenes = R.ragged_scenes(fixtures3, seeds=case["seeds"], fractional=case["fractional"])
    runner = R.EmulRunner(lib, scenes)
    assert runner.S.desc.grid_ne_binary == (0 if case["fractional"] else 1)
    q0, t0 = R.pose0(scenes)
    cache = {}
    fixed = {n: R.Fixed(runner, q0, t0, n, final_cache=cache) for n in case["steps"]}
    return dict(case=case, runner=runner, q0=q0, t0=t0, off=R.scene_offsets(scenes), fixed=fixed)


@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
def test_scenes_freeze_where_the_fixed_loop_says_bit_for_bit(ragged, parity):
    """n_steps equals the host mirror's; q, t, m, v of every scene are the fixed loop's at n_steps[s]; losses / traj
    rows before the stop are the fixed loop's, the rows after it still hold the pre-fill; the scene that never
    converges equals refine(max_iter); a replay of the same call gives the same bits (the observers start fresh).
    max_iter even and odd: a frozen scene's state ends in the caller's arrays from either copy."""
    case = ragged["case"]
    max_iter = [n for n in case["steps"] if n % 2 == parity][0]
    fixed = ragged["fixed"][max_iter]
    args = (ragged["runner"], ragged["q0"], ragged["t0"], max_iter, case["thr"], case["window"], case["n_pass"])
    got = R.run_converge(*args)
    want = R.assert_converged_like_fixed(got, fixed, ragged["off"], case["thr"], case["window"], case["n_pass"],
                                         expect=case["steps"][max_iter])
    assert (want == max_iter).sum() >= 1 and len(set(want)) == len(want)
    never = int(np.argmax(want == max_iter))
    lo, hi = ragged["off"][never], ragged["off"][never + 1]
    np.testing.assert_array_equal(R.bits(got["q"][lo:hi]), R.bits(fixed.final(max_iter)[0][lo:hi]))
    if parity == 0:
        again = R.run_converge(*args)
        for k in got:
            np.testing.assert_array_equal(R.bits(got[k]) if got[k].dtype == np.float32 else got[k],
                                          R.bits(again[k]) if again[k].dtype == np.float32 else again[k], err_msg=k)


def test_the_nodes_constants_and_a_later_adam_step(lib, fixtures3):
    """The node's rule as it stands (threshold 0.009, window 10, 3 passes) with step0 = 5, on the single-pass layout:
    whatever the mirror says over the fixed loop's losses, the device says."""
    scenes = R.ragged_scenes(fixtures3)
    runner = R.EmulRunner(lib, scenes)
    q0, t0 = R.pose0(scenes)
    fixed = R.Fixed(runner, q0, t0, 7, step0=5)
    got = R.run_converge(runner, q0, t0, 7, 0.009, 10, 3, step0=5)
    R.assert_converged_like_fixed(got, fixed, R.scene_offsets(scenes), 0.009, 10, 3)


def test_bad_arguments_are_refused(ragged, lib):
    r = ragged["runner"]
    q, t = ragged["q0"].copy(), ragged["t0"].copy()
    m, v = np.zeros((q.shape[0], 7), np.float32), np.zeros((q.shape[0], 7), np.float32)
    n_steps = np.full(r.n_scenes, -1, np.int32)
    common = (q, t, m, v, 4, 0, 0.01, 0.001, 0.009)
    assert r.converge_rc(*common, 17, 3, None, None, n_steps, r.observer) < 0   # window above the cap
    assert r.converge_rc(*common, 10, 3, None, None, n_steps, None) < 0         # no observer buffer
    assert r.converge_rc(*common, 10, 3, None, None, None, r.observer) < 0      # no n_steps
    assert (n_steps == -1).all() and (q == ragged["q0"]).all()
    assert lib.mf_icc_observer_bytes(3, 17) < 0 and lib.mf_icc_observer_bytes(0, 10) < 0
    assert lib.mf_icc_observer_bytes(3, 1) == lib.mf_icc_observer_bytes(3, 16) > 0
