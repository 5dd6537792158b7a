"""Group sets and worlds shared by the fleet tests (tests/test_fleet_host.py, tests/test_gpu_device_fleet.py)."""
import numpy as np


def limit_groups(B, Nother, seed=0):
    """Groups of ``B`` robots at the limits of the other-robot block: sizes 1, 2, ``Nother + 1`` (exactly full), ``Nother + 3``
    (truncated), one empty group, and the remaining robots as one group; every group's robots are scattered over 0..B-1 and
    out of order."""
    sizes = [1, 2, Nother + 1, Nother + 3]
    assert B > sum(sizes) + 1
    order = np.random.default_rng(seed).permutation(B)
    groups, at = [], 0
    for n in sizes:
        groups.append([int(i) for i in order[at:at + n]])
        at += n
    groups.insert(2, [])
    groups.append([int(i) for i in order[at:]])
    return groups


def other_groups(B, seed=1):
    """Another partition of the same robots: pairs (and one single when B is odd) -- every group of ``limit_groups`` with more
    than two robots shrinks."""
    order = [int(i) for i in np.random.default_rng(seed).permutation(B)]
    return [order[i:i + 2] for i in range(0, B, 2)]


def world(w, R, x_goal=10.0):
    """R robots of world w on crossing paths, the layout of tests/test_gpu_fleet.py (they meet half way)."""
    y0 = 3.0 + 0.3 * w
    starts = [np.array([0.6, y0 + 1.2 * r, 0.0]) for r in range(R)]
    goals = [np.array([x_goal, y0 + 1.2 * (R - 1 - r), 0.0]) for r in range(R)]
    paths = [[tuple(starts[r][:2]), tuple(goals[r][:2])] for r in range(R)]
    return starts, goals, paths
