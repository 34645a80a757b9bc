"""contrib.LossObserver: the stopping rule of the reference's collision-based pose refinement node
(collision_based_pose_refinement.py:18-45), against a hand-worked sequence and against the rule written out."""
import math

import numpy as np
import torch

from morefusion_amd.contrib import LossObserver


def _rule(losses, thr, window, n_pass):
    """The rule, literally: -> (n_passed after every add, index of the first add after which it validates)."""
    deltas, n_passed, out, stop = [], 0, [], None
    for i, x in enumerate(np.asarray(losses, np.float32)):
        if i >= 1:
            deltas.append(abs(float(np.float32(losses[i - 1])) - float(x)))
            deltas = deltas[-window:]
        if deltas:
            n_passed = n_passed + 1 if all(math.isfinite(d) and d < thr for d in deltas) else 0
        out.append(n_passed)
        if stop is None and n_passed >= n_pass:
            stop = i
    return out, stop


def test_hand_worked_sequence():
    """threshold 0.1, window 2, 2 passes.  losses 1.0, 0.5, 0.45, 0.44, 0.9, 0.89, 0.88, 0.87:
    deltas -, .5, .05, .01, .46, .01, .01, .01; windows -, [.5], [.5 .05], [.05 .01], [.01 .46], [.46 .01],
    [.01 .01], [.01 .01]; n_passed 0 0 0 1 0 0 1 2 -> validates after the eighth loss only."""
    ob = LossObserver(max_delta_threshold=0.1, window=2, n_passed_threshold=2)
    seen = []
    for x in (1.0, 0.5, 0.45, 0.44, 0.9, 0.89, 0.88, 0.87):
        ob.add(x)
        seen.append((ob._n_passed, ob.validate()))
    assert [s[0] for s in seen] == [0, 0, 0, 1, 0, 0, 1, 2]
    assert [s[1] for s in seen] == [False] * 7 + [True]


def test_first_loss_has_no_delta_and_the_defaults_stop_after_four():
    ob = LossObserver()
    assert (ob._max_delta_threshold, ob._n_passed_threshold, ob._deltas.maxlen) == (0.009, 3, 10)
    assert ob.add(0.25) is None and ob._last == 0.25 and len(ob._deltas) == 0 and ob._n_passed == 0
    for k, x in enumerate((0.25, 0.25, 0.25)):
        assert ob.add(torch.tensor(x)) == 0.0
        assert ob.validate() == (k == 2)  # the earliest stop: after the fourth step


def test_window_evicts_the_oldest_delta():
    ob = LossObserver(max_delta_threshold=0.1, window=3, n_passed_threshold=1)
    for x in (5.0, 1.0, 1.0, 1.0):   # deltas 4, 0, 0: the 4 is still in the window
        ob.add(x)
    assert not ob.validate() and list(ob._deltas) == [4.0, 0.0, 0.0]
    assert ob.add(1.0) == 0.0 and ob.validate()  # evicted


def test_one_large_delta_resets_n_passed():
    ob = LossObserver(max_delta_threshold=0.1, window=1, n_passed_threshold=3)
    for x in (1.0, 1.0, 1.0):
        ob.add(x)
    assert ob._n_passed == 2
    ob.add(2.0)
    assert ob._n_passed == 0 and not ob.validate()


def test_a_nan_in_the_window_fails_the_step_wherever_it_sits():
    """The stated departure from the node: Python's max([nan, 0.0]) is nan but max([0.0, nan]) is 0.0."""
    ob = LossObserver(max_delta_threshold=0.1, window=3, n_passed_threshold=1)
    for x in (1.0, float("nan"), 1.0, 1.0):  # deltas nan, nan, 0
        ob.add(x)
        assert ob._n_passed == 0
    assert math.isnan(ob.add(1.0))           # window [nan, 0, 0]
    assert ob._n_passed == 0
    ob.add(1.0)                              # [0, 0, 0]
    assert ob._n_passed == 1 and ob.validate()
    inf = LossObserver(max_delta_threshold=float("inf"), window=2, n_passed_threshold=1)
    inf.add(float("inf")); inf.add(1.0)
    assert inf._n_passed == 0


def test_against_the_rule_on_random_sequences():
    rs = np.random.RandomState(0)
    for trial in range(50):
        n, window, n_pass = rs.randint(2, 30), rs.randint(1, 6), rs.randint(1, 4)
        losses = np.cumsum(rs.normal(0, 0.01, n) * (rs.uniform(size=n) < 0.7)).astype(np.float32)
        if trial % 5 == 0:
            losses[rs.randint(n)] = np.nan
        ob = LossObserver(0.009, window, n_pass)
        got, stop = [], None
        for i, x in enumerate(losses):
            ob.add(x if i % 2 else np.float32(x))
            got.append(ob._n_passed)
            if stop is None and ob.validate():
                stop = i
        assert (got, stop) == _rule(losses, 0.009, window, n_pass)
