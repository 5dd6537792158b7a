"""Numpy twin of the prioritized K-step launch (include/mpcgpu_dqn_per.h): nothing but the two existing twins
composed -- ``per_numpy.SumTree.sample`` -> ``dqn_numpy.Twin.step(weights=...)`` -> ``SumTree.update`` -- around the uniform
draw, which is Python-integer arithmetic on the counter stream of ``dqn_numpy.sample_rows``."""
from __future__ import annotations

import numpy as np

from . import dqn_numpy as tw

F = np.float32
_MASK = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def draw_bits(seed: int, serial: int, n: int) -> list:
    """bits_i = mix64(mix64(seed + G * serial) + G * (i + 1)), i = 0 .. n - 1, as Python integers."""
    key = tw.mix64((seed + _G * serial) & _MASK)
    return [tw.mix64((key + _G * (i + 1)) & _MASK) for i in range(n)]


def uniform_of(bits: int) -> float:
    """(double)(bits >> 11) * 2^-53: both the conversion (53 bits) and the scaling are exact."""
    return float(bits >> 11) * 2.0 ** -53


def uniforms(seed: int, serial: int, n: int) -> np.ndarray:
    return np.array([uniform_of(b) for b in draw_bits(seed, serial, n)], dtype=np.float64)


def train_per(twin, tree, buf, n_entries, n, k, seed, serial0, after_step=None):
    """``twin``: dqn_numpy.Twin, ``tree``: per_numpy.SumTree, ``buf``: dict of the buffer's five arrays (capacity rows each)
    -> (losses [k], tree indices [k, n], delta [k, n]).  ``after_step(s, indices, positions, tree_before)`` is called after
    every step."""
    losses, indices, delta = np.zeros(k, F), np.zeros((k, n), np.int64), np.zeros((k, n), F)
    for s in range(k):
        before = tree.tree.copy() if after_step is not None else None
        idx, pos, w = tree.sample(uniforms(seed, serial0 + s, n), n_entries)
        _, losses[s], delta[s] = twin.step(buf["obs"][pos], buf["next_obs"][pos], buf["actions"][pos], buf["rewards"][pos],
                                           buf["dones"][pos], weights=w.astype(F))
        tree.update(idx, delta[s])
        indices[s] = idx
        if after_step is not None:
            after_step(s, idx, pos, before)
    return losses, indices, delta
