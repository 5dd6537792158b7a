#!/usr/bin/env python3
"""The slow half of the planner's limit tests, recorded: the twin's and the brute force's results on the large maps.

Run:   python tests/golden/make_planner_limits_fixture.py        (about ten minutes on eight cores)

For every map of ``tests.support.plan_maps.limit_maps()`` -- the eight start/goal pairs of ``field_of_polygons``, the three
``saw_hall``s, ``walled_field`` and the six ``tie_square``s -- the twin (tests/support/plan_numpy.py) needs seconds and the
brute-force check (tests/support/plan_bruteforce.py) up to minutes, so the tests read what both gave from here and
recompute only part of it (tests/test_plan_restatement.py says which part).  Nothing but this repository is needed.

Before anything is written the twin must agree with the brute force within the bound of
``test_plan_restatement.check_against_bruteforce``: |twin - brute| <= 1e-9 brute, nan against status 2, inf against status 1.

Written: planner_limits.npz -- results only, the maps are rebuilt from their builders
  names         the maps, in ``limit_maps()`` order
  twin_status / twin_n_nodes / twin_nodes [M, 64, 2] / twin_length      at n_node_max = 64
  brute_length  nan: start or goal not free; inf: no path; for status 3 the length of the path that is too long
"""
import math
import multiprocessing
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.support import plan_bruteforce as brute  # noqa: E402
from tests.support import plan_maps  # noqa: E402
from tests.support import plan_numpy as twin  # noqa: E402


def both(index):
    name, m = plan_maps.limit_maps()[index]
    r = twin.plan(*m)
    want = brute.shortest_length(*m)
    print(f"{name}: twin status {r['status']} nodes {r['n_nodes']} length {r['length']!r}; brute force {want!r}", flush=True)
    return r, want


if __name__ == "__main__":
    names = [name for name, _ in plan_maps.limit_maps()]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(both, range(len(names)), chunksize=1)
    M = len(names)
    status, n_nodes = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
    nodes, length, brute_length = np.zeros((M, 64, 2)), np.zeros(M), np.zeros(M)
    for i, (r, want) in enumerate(results):
        if math.isnan(want):
            assert r["status"] == twin.NOT_FREE, names[i]
        elif math.isinf(want):
            assert r["status"] == twin.NO_PATH, names[i]
        elif r["status"] == twin.TOO_MANY_NODES:
            assert r["n_nodes"] > 64, names[i]          # the twin keeps no length for it: nothing to compare
        else:
            assert r["status"] == twin.OK and abs(r["length"] - want) <= 1e-9 * want, names[i]
        status[i], n_nodes[i], length[i], brute_length[i] = r["status"], r["n_nodes"], r["length"], want
        nodes[i, :len(r["nodes"])] = r["nodes"]
    np.savez_compressed(os.path.join(HERE, "planner_limits.npz"), names=np.array(names), twin_status=status, twin_n_nodes=n_nodes,
                        twin_nodes=nodes, twin_length=length, brute_length=brute_length)
    print("wrote planner_limits.npz")
