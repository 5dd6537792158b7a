"""TEST INFRASTRUCTURE -- environments on the two-record table for the tests of collection with map turnover
(tests/test_gpu_collect_fresh.py), on the maps of tests/support/collect_cases.py.

Row b starts on ``collect_cases.maps(B)[b]``, a map of kind ``b % 3``; its spare is a map of kind ``(b + 1) % 3`` from a
stream of its own, so a row that turns over changes kind.  With ``max_episode_steps = 3`` every episode on either map ends
within three steps whatever the actions."""
from __future__ import annotations

import numpy as np

from oracle import rl_env_numpy as orc
from trajtrack_mpcndqn_rlboost_amd import rl_env

from . import collect_cases as cc

_SPARES = {}


def spare_maps(B: int):
    """The spare of every row: row b's is ``collect_cases.one_map`` of kind ``(b + 1) % 3`` (built once per process)."""
    if B not in _SPARES:
        rng = np.random.default_rng(7000 + B)
        _SPARES[B] = [cc.one_map(rng, (b + 1) % 3) for b in range(B)]
    return _SPARES[B]


_FIRST = {}


def first_step_endings(B: int) -> np.ndarray:
    """[B] bool: whether row b's first episode on ``collect_cases.maps(B)`` ends at its first step, by the numpy oracle on the
    CPU.  It does not depend on the action (asserted): every row of kind 1, no row of kind 0, and those rows of kind 2 whose
    start, 0.85 m from a goal at a wall, lies inside the padded wall (7 of 64, row 2 among them)."""
    if B not in _FIRST:
        ends = np.array([[bool(orc.OracleRaysEnv(m).step(a)[2]) for a in range(9)] for m in cc.maps(B)])
        assert (ends == ends[:, :1]).all()
        kinds = np.arange(B) % 3
        assert ends[kinds == 1].all() and not ends[kinds == 0].any()
        _FIRST[B] = ends[:, 0]
    return _FIRST[B]


def capacity(B: int):
    """Limits of a record table that holds the start maps and the spares."""
    return rl_env.pack_records(list(cc.maps(B)) + list(spare_maps(B)))[1]


def stream_capacity(B: int):
    """Limits that hold ``collect_cases.maps(B)`` (obstacles of three key frames) AND the maps of the stream."""
    from trajtrack_mpcndqn_rlboost_amd import map_stream
    own = rl_env.pack_records(list(cc.maps(B)))[1]
    return {k: max(v, own[k]) for k, v in map_stream.DYNAMIC_CAPACITY.items()}


def make_env(B: int, spare_rows=None):
    """``collect_cases.maps(B)`` after ``enable_spares()`` and a reset; ``spare_rows`` (default: the even rows) get their spare
    loaded, the others have none."""
    env = rl_env.BatchedRaysEnv(cc.maps(B), max_episode_steps=cc.MAX_EPISODE_STEPS, capacity=capacity(B))
    env.enable_spares()
    env.reset()
    rows = list(range(0, B, 2)) if spare_rows is None else list(spare_rows)
    env.load_spares(rows, [spare_maps(B)[b] for b in rows])
    return env
