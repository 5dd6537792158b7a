"""Numpy twin of the action rule of include/mpcgpu_collect.h (csrc/dqn_act.hpp): ``dqn_numpy.network`` for the
nine values, the scan with a strict ``>`` for the greedy action, Python integers for the two draws of a row."""
from __future__ import annotations

import numpy as np

from . import dqn_numpy as tw

F = np.float32
_MASK, _G = tw._MASK, tw._G


def draw_bits(seed: int, serial: int, b: int):
    """(bits_e, bits_a) of row ``b`` at step ``serial`` of stream ``seed``."""
    key = tw.mix64((seed + _G * serial) & _MASK)
    return tw.mix64((key + _G * (2 * b + 1)) & _MASK), tw.mix64((key + _G * (2 * b + 2)) & _MASK)


def uniform_of(bits: int) -> float:
    """(bits >> 11) * 2^-53: exact in float64."""
    return float(bits >> 11) * 2.0 ** -53


def random_of(bits: int) -> int:
    """The high half of the 128-bit product bits * 9."""
    return (bits * 9) >> 64


def greedy(q) -> np.ndarray:
    """Row-wise scan of ``q`` [n, 9]: start at 0, take a when q[a] > q[greedy]."""
    q = np.asarray(q)
    best, val = np.zeros(q.shape[0], np.int64), q[:, 0].copy()
    for a in range(1, q.shape[1]):
        better = q[:, a] > val
        best, val = np.where(better, a, best), np.where(better, q[:, a], val)
    return best


def flat(external, internal) -> np.ndarray:
    return np.concatenate([np.asarray(external, F), np.asarray(internal, F)], axis=1)


def act(theta, x, eps: float, seed: int, serial: int):
    """``x`` [B, 46] float32 -> (actions int32 [B], q float32 [B, 9], explored bool [B], u float64 [B])."""
    x = np.asarray(x, F)
    q = tw.network(np.asarray(theta, F)[:tw.NP], x)[2]
    g = greedy(q)
    B = x.shape[0]
    bits = [draw_bits(seed, serial, b) for b in range(B)]
    u = np.array([uniform_of(e) for e, _ in bits], np.float64).reshape(B)
    explore = u < float(eps)
    rnd = np.array([random_of(a) for _, a in bits], np.int64).reshape(B)
    return np.where(explore, rnd, g).astype(np.int32), q, explore, u
