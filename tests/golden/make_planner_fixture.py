#!/usr/bin/env python3
"""The reference's twelve ``generate_map_mpc`` maps as planner inputs, with the TWIN's paths beside them.

Run in the build container only (needs /root/reference):   python tests/golden/make_planner_fixture.py

The reference's own map generator (src/pkg_dqn/utils/map.py:20-155) is imported and called with the shims of
``make_env_fixtures.py`` (gym, cv2, extremitypathfinder, a small shapely); from the objects it returns, the boundary
vertices, the outlines of the obstacles that are visible on the reference path, the robot's start position and the goal
are read.  No program text of the reference is copied: the coordinates reach the repository only as this data file.

Written: planner_maps.npz
  specs_json   the 12 maps: boundary, static, start, goal (numbers only)
  twin_status / twin_n_nodes / twin_nodes [12, 64, 2] / twin_length
               the paths of tests/support/plan_numpy.py on the maps inflated as environment.py:130-140 does (obstacles
               0.8, boundary 0.5, mitred).  They are RECORDED RESULTS OF THE TWIN, NOT OF THE REFERENCE: its planner
               (extremitypathfinder) is not installed here.  tests/tools/planner_pin.py is the way to pin them.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_env_fixtures import install_shims  # noqa: E402

N_MAPS = 12

if __name__ == "__main__":
    install_shims()
    sys.path.insert(0, os.path.join(REF, "src"))
    import importlib
    map_mod = importlib.import_module("pkg_dqn.utils.map")
    from tests.support import plan_numpy as twin
    from trajtrack_mpcndqn_rlboost_amd import path_plan

    specs = []
    for i in range(N_MAPS):
        robot, boundary, obstacles, goal = map_mod.generate_map_mpc(i)()
        specs.append(dict(boundary=np.asarray(boundary.vertices, dtype=np.float64).tolist(),
                          static=[np.asarray(o.nodes, dtype=np.float64).tolist() for o in obstacles if o.visible_on_reference_path],
                          start=np.asarray(robot.position, dtype=np.float64).tolist(),
                          goal=np.asarray(goal.position, dtype=np.float64).tolist()))
    status = np.zeros(N_MAPS, dtype=np.int32)
    n_nodes = np.zeros(N_MAPS, dtype=np.int32)
    nodes = np.zeros((N_MAPS, 64, 2))
    length = np.zeros(N_MAPS)
    for i, sp in enumerate(specs):
        b, obs = path_plan.inflate_spec(sp)
        r = twin.plan(path_plan.oriented_rings(b, obs), sp["start"], np.asarray(sp["goal"], dtype=np.float32).astype(np.float64))
        status[i], n_nodes[i], length[i] = r["status"], r["n_nodes"], r["length"]
        nodes[i, :len(r["nodes"])] = r["nodes"]
        print(i, "status", r["status"], "nodes", r["n_nodes"], "length", r["length"])
    np.savez_compressed(os.path.join(HERE, "planner_maps.npz"),
                        specs_json=np.frombuffer(json.dumps(specs).encode(), dtype=np.uint8),
                        twin_status=status, twin_n_nodes=n_nodes, twin_nodes=nodes, twin_length=length,
                        paths_are=np.array("output of tests/support/plan_numpy.py (the twin), not of the reference's planner"))
    print("wrote planner_maps.npz")
