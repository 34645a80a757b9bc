"""LossObserver -- the stopping rule of the reference's collision-based pose refinement node.

ros/src/morefusion_ros/nodes/collision_based_pose_refinement.py:18-45: the node feeds the loss of every
iteration (after ``optimizer.update()``) to ``add`` and leaves its loop of at most 30 iterations once
``validate()`` holds.  Same attribute names, same constants.  This is the host class: what a caller of the
host-loop ``IterativeCollisionCheckLink.forward`` needs to run the node's loop, and the mirror of the per-scene
observers that ``IccScenes.refine_until_converged`` keeps on the device (csrc/icc_step.h: icc_obs_advance).

One stated departure from the node, shared with the device: while the window holds a non-finite delta the step
does not pass and ``_n_passed`` is reset.  The node takes Python's ``max`` of the window, whose answer for a list
holding a NaN depends on where the NaN sits.
"""
import collections
import math

import numpy as np


class LossObserver:
    def __init__(self, max_delta_threshold=0.009, window=10, n_passed_threshold=3):
        self._last = None
        self._deltas = collections.deque([], int(window))
        self._n_passed = 0

        self._max_delta_threshold = float(max_delta_threshold)
        self._n_passed_threshold = int(n_passed_threshold)

    def add(self, loss):
        """``loss``: a float, a NumPy scalar or a 0-d tensor / variable (the node passes ``loss`` itself).  The value
        is taken as float32, what the loss is on the device.  Returns the window's largest delta (None while the
        window is empty; NaN if a delta is NaN)."""
        if hasattr(loss, "array"):  # (chainer.Variable, as in the node)
            loss = loss.array
        loss = float(np.float32(loss.item() if hasattr(loss, "item") else loss))

        if self._last is not None:
            delta = abs(self._last - loss)
            self._deltas.append(delta)
        self._last = loss

        max_delta = None
        if self._deltas:
            finite = all(math.isfinite(d) for d in self._deltas)
            max_delta = max(self._deltas) if finite else (
                float("nan") if any(math.isnan(d) for d in self._deltas) else float("inf"))
            if finite and max_delta < self._max_delta_threshold:
                self._n_passed += 1
            else:
                self._n_passed = 0
        return max_delta

    def validate(self):
        return self._n_passed >= self._n_passed_threshold
