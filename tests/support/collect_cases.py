"""TEST INFRASTRUCTURE -- environments for the tests of collection inside one launch (tests/test_gpu_collect.py).

:func:`maps` draws ``env_maps.random_map`` halls and gives every row one of three starts, chosen with the numpy oracle
(oracle/rl_env_numpy.py) on the CPU, so that with ``max_episode_steps = 3`` a launch of a few steps holds episodes that end both
ways:

* row kind 0, *time limit*: a free spot away from the goal, at rest -- whatever it does, it moves less than 0.3 m in three
  steps; the oracle confirms that three steps of full acceleration, of coasting and of full braking end neither in a collision
  nor at the goal, so the episode is truncated at its third step;
* row kind 1, *terminal at once*: 0.6 m from the goal, heading for it at 1 m/s -- the first step ends the episode, at the goal
  or, where the goal lies at a wall, in the wall;
* row kind 2, *terminal later*: 0.85 m from the goal, heading for it at 1 m/s -- the episode ends at its second or third step,
  depending on the actions.

Row b is of kind b mod 3.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import rl_env_numpy as orc

from . import env_maps

MAX_EPISODE_STEPS = 3
KINDS = ("time limit", "terminal at once", "terminal later")


def _quiet(m, start) -> bool:
    """Three steps from ``start`` under full acceleration, coasting and full braking end nowhere."""
    for action in (0, 4, 8, 2, 6):
        o = orc.OracleRaysEnv(dict(m, start=np.asarray(start, dtype=np.float64)))
        if o.collided or o.reached_goal:
            return False
        for _ in range(MAX_EPISODE_STEPS):
            if o.step(action)[2]:
                return False
    return True


def one_map(rng, kind: int):
    while True:
        m = env_maps.random_map(rng, n_obst=(0, 4))
        gx, gy = float(m["goal"][0]), float(m["goal"][1])
        if kind == 0:
            ring = np.asarray(m["boundary_padded"])
            for _ in range(20):
                x, y = rng.uniform(ring[:, 0].min() + 1.0, ring[:, 0].max() - 1.0), rng.uniform(ring[:, 1].min() + 1.0, ring[:, 1].max() - 1.0)
                start = [float(x), float(y), float(rng.uniform(-math.pi, math.pi)), 0.0, 0.0]
                if math.hypot(x - gx, y - gy) > 2.0 and _quiet(m, start):
                    return dict(m, start=np.asarray(start))
            continue
        ang = float(rng.uniform(-math.pi, math.pi))
        d = 0.6 if kind == 1 else 0.85
        start = [gx + d * math.cos(ang), gy + d * math.sin(ang), ang + math.pi, 1.0, 0.0]      # heading for the goal
        return dict(m, start=np.asarray(start))


_CACHE = {}


def maps(B: int, seed: int = 0):
    """B maps, row b of kind b mod 3; the same list for the same arguments (built once per process)."""
    if (B, seed) not in _CACHE:
        rng = np.random.default_rng(1000 + seed)
        _CACHE[(B, seed)] = [one_map(rng, b % 3) for b in range(B)]
    return _CACHE[(B, seed)]


def mixed_eps(T: int):
    """Epsilons of one launch: 1.0, 0.0, 0.37, then a ramp -- explored and greedy steps, and steps that are both."""
    base = [1.0, 0.0, 0.37]
    return [base[t] if t < 3 else 0.05 + 0.9 * ((7 * t) % 10) / 10.0 for t in range(T)]
