#!/usr/bin/env python3
"""Pin the restated path planner and the restated mitred buffer against the REAL libraries -- on a machine that has them.

Why this file exists.  The reference plans its reference path with ``extremitypathfinder`` on outlines mitred by shapely
(``src/pkg_dqn/environment/environment.py:122-146``, ``obstacle.py:177-185,248-256``).  Neither is a dependency of this
project, so ``rl_geometry.mitre_polygon`` restates the buffer and ``tests/support/plan_numpy.py`` (and the HIP kernel that
follows it) the planner: "parity unpinned" (DESIGN.md section 8.3).  This script is the missing link.  It never runs on
the GPU box and imports nothing from the GPU package but the host-side geometry.

  step 1 (a machine WITH extremitypathfinder and shapely):
      python tests/tools/planner_pin.py record [--out planner_pin.npz] [--n 200] [--seed 0]
    for the 12 maps of tests/golden/planner_maps.npz and ``n`` seeded ``rl_env.random_dynamic_spec`` maps: shapely's
    ``Polygon.buffer(d, join_style=mitre, mitre_limit=2)`` of every static obstacle (0.8) and of the boundary (-0.5), and
    ``PolygonEnvironment.store(..., validate=False); prepare(); find_shortest_path(start, goal)`` on those rings.

  step 2 (any machine with this repository; no shapely, no GPU):
      python tests/tools/planner_pin.py compare planner_pin.npz
    runs ``mitre_polygon`` and the twin on every recorded map and prints how many rings agree (as vertex sets, 1e-9) and
    how many paths agree in length (1e-9 relative) and in their nodes; for the first mismatch of each kind, the map.
    Overlapping inflated obstacles and obstacles across the boundary are where the library's answer is least certain
    (it is documented for non-overlapping holes): a mismatch there says what the reference really trains on.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def specs_of(n: int, seed: int):
    import importlib
    rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "planner_maps.npz"))
    specs = json.loads(bytes(fx["specs_json"]).decode())
    rng = np.random.default_rng(seed)
    for _ in range(n):
        s = rl_env.random_dynamic_spec(rng)
        specs.append(dict(boundary=s["boundary"], static=s["static"], start=s["start"][:2], goal=s["goal"]))
    return specs


def record(args) -> None:
    try:
        from extremitypathfinder import PolygonEnvironment
        from shapely.geometry import JOIN_STYLE, Polygon
    except ImportError:
        sys.exit("record needs extremitypathfinder and shapely: run it on a machine that has them; `compare` then runs anywhere")
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # noqa: E731

    def ring(poly, clockwise):
        ext = poly.exterior
        coords = ext.coords[-2::-1] if ext.is_ccw == clockwise else ext.coords[:-1]
        return np.asarray(coords, dtype=np.float64)

    out = []
    for sp in specs_of(args.n, args.seed):
        obstacles = [ring(Polygon(f32(o)).buffer(0.8, join_style=JOIN_STYLE.mitre, mitre_limit=2), True) for o in sp["static"]]
        boundary = ring(Polygon(f32(sp["boundary"])).buffer(-0.5, join_style=JOIN_STYLE.mitre, mitre_limit=2), False)
        env = PolygonEnvironment()
        path, length = [], None
        try:
            env.store(boundary, obstacles, validate=False)
            env.prepare()
            path, length = env.find_shortest_path(tuple(sp["start"][:2]), tuple(f32(sp["goal"])[:2]))
            error = None
        except Exception as exc:          # the library may refuse overlapping holes: that is part of the answer
            error = repr(exc)
        out.append(dict(spec=sp, boundary=boundary.tolist(), obstacles=[o.tolist() for o in obstacles],
                        path=np.asarray(path, dtype=np.float64).reshape(-1, 2).tolist(), length=length, error=error))
    import extremitypathfinder
    import shapely
    np.savez_compressed(args.out, recording=np.frombuffer(json.dumps(out).encode(), dtype=np.uint8),
                        versions=np.array(f"extremitypathfinder {getattr(extremitypathfinder, '__version__', '?')}, shapely {shapely.__version__}"))
    print(f"wrote {args.out}: {len(out)} maps")


def compare(args) -> None:
    from tests.support import plan_numpy as twin
    from trajtrack_mpcndqn_rlboost_amd import path_plan

    def same_ring(a, b):
        a, b = np.asarray(a).reshape(-1, 2), np.asarray(b).reshape(-1, 2)
        return len(a) == len(b) and all(np.min(np.hypot(*(b - p).T)) <= 1e-9 for p in a)

    d = np.load(args.recording)
    rec = json.loads(bytes(d["recording"]).decode())
    rings_ok = paths_ok = nodes_ok = refused = 0
    first_ring = first_path = None
    for i, r in enumerate(rec):
        mine_b, mine_o = path_plan.inflate_spec(r["spec"])
        good = same_ring(mine_b, r["boundary"]) and len(mine_o) == len(r["obstacles"]) and \
            all(same_ring(a, b) for a, b in zip(mine_o, r["obstacles"]))
        rings_ok += good
        if not good and first_ring is None:
            first_ring = i
        if r["error"] is not None:
            refused += 1
            continue
        # the planner on the LIBRARY's rings, so that a buffer mismatch does not hide a planner match
        res = twin.plan(path_plan.oriented_rings(r["boundary"], r["obstacles"]), r["spec"]["start"][:2],
                        np.asarray(r["spec"]["goal"], dtype=np.float32).astype(np.float64)[:2])
        theirs = np.asarray(r["path"]).reshape(-1, 2)
        if (res["status"] != 0) == (len(theirs) == 0) and (res["status"] != 0 or abs(res["length"] - r["length"]) <= 1e-9 * r["length"]):
            paths_ok += 1
            nodes_ok += res["status"] != 0 or (len(theirs) == res["n_nodes"] and bool(np.allclose(theirs, res["nodes"], atol=1e-9)))
        elif first_path is None:
            first_path = i
    n = len(rec)
    print(f"{d['versions']}: {n} maps; mitred rings equal on {rings_ok}; the library planned {n - refused} (refused {refused}); "
          f"path length equal on {paths_ok}, nodes equal on {nodes_ok}")
    for what, i in (("ring", first_ring), ("path", first_path)):
        if i is not None:
            print(f"first {what} mismatch: map {i}: {json.dumps(rec[i])[:2000]}")
    sys.exit(0 if rings_ok == n and paths_ok == n - refused else 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--out", default="planner_pin.npz")
    r.add_argument("--n", type=int, default=200)
    r.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("compare")
    c.add_argument("recording")
    args = ap.parse_args()
    record(args) if args.cmd == "record" else compare(args)


if __name__ == "__main__":
    main()
