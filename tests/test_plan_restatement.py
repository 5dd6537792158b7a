"""The visibility-graph planner without a GPU: analytic cases of the twin (tests/support/plan_numpy.py), the
twin against an independent brute-force check (tests/support/plan_bruteforce.py), ``rl_geometry.mitre_polygon``, and the
C header against ``path_plan.PLAN_EXPORTS`` and the built library."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest

from tests.support import plan_bruteforce as brute
from tests.support import plan_maps
from tests.support import plan_numpy as twin
from trajtrack_mpcndqn_rlboost_amd import path_plan, rl_env
from trajtrack_mpcndqn_rlboost_amd import rl_geometry as rg

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")  # (the package attribute `solver` is the plugin factory)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = [(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0)]


def box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


# ---- analytic cases -----------------------------------------------------------------------------------------------------
def test_empty_room_is_the_straight_line():
    r = twin.plan(path_plan.oriented_rings(ROOM, []), (1.0, 2.0), (9.0, 7.5))
    assert r["status"] == twin.OK and r["n_nodes"] == 2
    assert r["nodes"].tolist() == [[1.0, 2.0], [9.0, 7.5]]
    assert r["length"] == math.sqrt(8.0 * 8.0 + 5.5 * 5.5)


def test_one_square_in_the_way_goes_round_one_corner():
    r = twin.plan(path_plan.oriented_rings(ROOM, [box(3, 2, 7, 6)]), (1.0, 1.0), (9.0, 8.0))
    assert r["status"] == twin.OK and r["n_nodes"] == 3
    assert r["nodes"].tolist() == [[1.0, 1.0], [3.0, 6.0], [9.0, 8.0]]
    assert r["length"] == math.sqrt(29.0) + math.sqrt(40.0)


def test_symmetric_square_takes_the_corner_with_the_lower_node_index():
    """Both ways round a square centred between start and goal are equally long, bit for bit.  The tie rule: the corner
    that comes first in table order is settled first and relaxes the goal; the other cannot replace it (strict <)."""
    rings = path_plan.oriented_rings(ROOM, [box(3, 3, 7, 7)])
    r = twin.plan(rings, (1.0, 1.0), (9.0, 9.0))
    assert r["status"] == twin.OK and r["n_nodes"] == 3
    table = rings[1].tolist()
    first = min(([7.0, 3.0], [3.0, 7.0]), key=table.index)
    assert r["nodes"][1].tolist() == first
    assert r["length"] == math.sqrt(40.0) + math.sqrt(40.0)
    # and the reference's first training map is such a tie (a square centred between start and goal)
    _, maps, fx = plan_maps.fixture()
    r0 = twin.plan(*maps[0])
    assert maps[0][1].tolist() == [1.0, 1.0] and maps[0][2].tolist() == [8.0, 8.0]
    corners = [v for v in maps[0][0][1].tolist() if v[0] != v[1]]          # the two corners off the diagonal, in table order
    a, b = corners
    assert a == b[::-1]                                                    # mirror images: both ways are equally long
    assert r0["n_nodes"] == 3 and r0["nodes"][1].tolist() == a


def test_concave_boundary_of_the_fixture_bends_at_boundary_corners():
    specs, maps, _ = plan_maps.fixture()
    rings, start, goal = maps[2]                       # the 16-vertex hall
    assert len(rings[0]) == 16
    r = twin.plan(rings, start, goal)
    assert r["status"] == twin.OK
    on_boundary = [p for p in r["nodes"][1:-1].tolist() if p in rings[0].tolist()]
    assert len(on_boundary) >= 3
    for p, q in zip(r["nodes"][:-1], r["nodes"][1:]):
        assert brute.segment_is_free(p, q, rings)


def test_goal_inside_an_obstacle_is_status_2():
    rings = path_plan.oriented_rings(ROOM, [box(3, 2, 7, 6)])
    assert twin.plan(rings, (1.0, 1.0), (5.0, 4.0))["status"] == twin.NOT_FREE
    assert twin.plan(rings, (-1.0, 1.0), (9.0, 4.0))["status"] == twin.NOT_FREE       # start outside the boundary
    assert twin.plan(rings, (1.0, 1.0), (7.0, 4.0))["status"] == twin.OK              # on the outline is free


def test_goal_walled_off_is_status_1():
    r = twin.plan(path_plan.oriented_rings(ROOM, [box(4, -1, 6, 11)]), (1.0, 5.0), (9.0, 5.0))
    assert r["status"] == twin.NO_PATH and r["n_nodes"] == 0 and r["length"] == 0.0


def test_start_equal_to_goal():
    r = twin.plan(path_plan.oriented_rings(ROOM, [box(3, 2, 7, 6)]), (1.0, 1.0), (1.0, 1.0))
    assert r["status"] == twin.OK and r["n_nodes"] == 2 and r["length"] == 0.0
    assert r["nodes"].tolist() == [[1.0, 1.0], [1.0, 1.0]]


def test_running_along_edges_and_through_touching_corners_is_allowed():
    """Two boxes that share a corner point, and a path that must run along a full edge."""
    rings = path_plan.oriented_rings(ROOM, [box(2, 0, 4, 5), box(4, 5, 6, 10)])
    assert twin.plan(rings, (1.0, 5.0), (9.0, 5.0))["status"] == twin.OK               # through the touching corner (4, 5)
    rings = path_plan.oriented_rings(ROOM, [box(2, -1, 4, 5), box(4, 5, 6, 11), box(3, 4, 5, 6)])
    assert twin.plan(rings, (1.0, 5.0), (9.0, 5.0))["status"] == twin.NO_PATH          # a third box plugs the corner
    r = twin.plan(path_plan.oriented_rings(ROOM, [box(3, -1, 7, 6)]), (3.0, 1.0), (7.0, 1.0))
    assert r["nodes"].tolist() == [[3.0, 1.0], [3.0, 6.0], [7.0, 6.0], [7.0, 1.0]] and r["length"] == 14.0


def test_limit_maps_have_the_node_counts_they_are_built_for():
    assert twin.plan(*plan_maps.zigzag(62))["n_nodes"] == 64
    r = twin.plan(*plan_maps.zigzag(63))
    assert r["status"] == twin.TOO_MANY_NODES and r["n_nodes"] == 65
    assert sum(len(r) for r in plan_maps.many_vertices(256)[0]) == 256
    assert len(plan_maps.comb_of_boxes()[0]) == 32


# ---- twin against brute force -----------------------------------------------------------------------------------------------
def check_against_bruteforce(rings, start, goal):
    r = twin.plan(rings, start, goal)
    want = brute.shortest_length(rings, start, goal)
    print(f"twin status {r['status']} nodes {r['n_nodes']} length {r['length']!r}; brute force {want!r}")
    if math.isnan(want):
        assert r["status"] == twin.NOT_FREE
    elif math.isinf(want):
        assert r["status"] == twin.NO_PATH
    else:
        assert r["status"] == twin.OK
        # float64 summation of at most 64 terms, not a measured tolerance
        assert abs(r["length"] - want) <= 1e-9 * want
        for p, q in zip(r["nodes"][:-1], r["nodes"][1:]):
            assert brute.segment_is_free(p, q, rings), (p, q)
    return r


@pytest.mark.parametrize("index", range(12))
def test_twin_equals_bruteforce_on_the_fixture_maps(index):
    _, maps, fx = plan_maps.fixture()
    r = check_against_bruteforce(*maps[index])
    # the recorded results are the twin's own (not the reference's): the file and the code must not drift apart
    assert r["status"] == fx["twin_status"][index] and r["n_nodes"] == fx["twin_n_nodes"][index]
    assert np.array_equal(r["nodes"], fx["twin_nodes"][index, :r["n_nodes"]]) and r["length"] == fx["twin_length"][index]
    assert "twin" in str(fx["paths_are"]) and "not of the reference" in str(fx["paths_are"])


def test_twin_equals_bruteforce_on_seeded_random_dynamic_maps():
    n = 200
    maps, draws, discarded = plan_maps.random_maps(seed=2024, n=n)
    print(f"{draws} draws, {discarded} discarded for a near-collinear triple")
    assert draws - discarded == n and discarded <= 0.10 * draws
    crossing = overlapping = 0
    status = []
    for rings, start, goal in maps:
        status.append(check_against_bruteforce(rings, start, goal)["status"])
        crossing += any(r[:, 1].min() < rings[0][:, 1].min() or r[:, 1].max() > rings[0][:, 1].max() for r in rings[1:])
        boxes = [(r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()) for r in rings[1:]]
        overlapping += any(a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
                           for i, a in enumerate(boxes) for b in boxes[i + 1:])
    # the generator reaches what it is meant to reach
    assert crossing >= 20 and overlapping >= 20 and status.count(twin.OK) >= 150


def test_twin_equals_bruteforce_on_a_ring_of_boxes_across_the_boundary():
    check_against_bruteforce(*plan_maps.comb_of_boxes(7))


# ---- mitre_polygon ---------------------------------------------------------------------------------------------------------------
def test_mitre_square_grows_to_the_square_with_side_plus_2d():
    out = rg.mitre_polygon(box(1, 1, 4, 4), 0.8)
    assert np.allclose(sorted(out.tolist()), sorted(box(0.2, 0.2, 4.8, 4.8)), atol=1e-15)
    assert rg.signed_area(out) > 0
    inner = rg.mitre_polygon(box(0, 0, 10, 10), -0.5)
    assert np.allclose(sorted(inner.tolist()), sorted(box(0.5, 0.5, 9.5, 9.5)), atol=1e-15)


def test_mitre_of_a_20_degree_corner_is_bevelled_at_2d():
    d, half = 0.5, math.radians(10.0)
    tri = [(0.0, 0.0), (10.0 * math.cos(half), -10.0 * math.sin(half)), (10.0 * math.cos(half), 10.0 * math.sin(half))]
    out = rg.mitre_polygon(tri, d)
    assert d / math.sin(half) > 2.0 * d                     # the full mitre would reach d / sin(10 deg) = 5.76 d from the apex
    assert len(out) == 4                                    # the apex became two points, the 80 degree corners stayed mitred
    near = out[np.argsort(out[:, 0])[:2]]
    assert np.allclose(near[:, 0], -2.0 * d, atol=1e-12)    # the bevel: perpendicular to the bisector, 2 d from the apex
    assert np.allclose(sorted(near[:, 1]), [-(d - 2 * d * math.sin(half)) / math.cos(half), (d - 2 * d * math.sin(half)) / math.cos(half)],
                       atol=1e-12)                          # and its ends lie on the two offset edges
    assert len(rg.mitre_polygon(tri, d, mitre_limit=6.0)) == 3
    assert np.allclose(rg.mitre_polygon(tri, d, mitre_limit=6.0)[:, 0].min(), -d / math.sin(half), atol=1e-12)


def test_mitre_shrinking_a_boundary_that_pinches_raises():
    hourglass = [(0.0, 0.0), (10.0, 0.0), (10.0, 4.0), (5.6, 4.6), (10.0, 5.2), (10.0, 10.0), (0.0, 10.0), (0.0, 5.2), (4.4, 4.6),
                 (0.0, 4.0)]
    assert rg.ring_is_simple(np.asarray(hourglass))
    rg.mitre_polygon(hourglass, -0.2)                       # the neck (1.2 wide) survives 0.2
    with pytest.raises(ValueError):
        rg.mitre_polygon(hourglass, -0.8)


def test_random_dynamic_spec_follows_the_reference_distributions():
    rng = np.random.default_rng(1)
    for _ in range(50):
        s = rl_env.random_dynamic_spec(rng)
        assert len(s["static"]) == 3 and len(s["dynamic"]) == 7 and s["start"][0] == 5.0 and s["goal"][0] == 35.0
        assert 5 <= s["start"][1] <= 15 and 5 <= s["goal"][1] <= 15 and s["start"][3:] == [0.0, 0.0]
        for b in s["static"]:
            w, h = b[1][0] - b[0][0], b[2][1] - b[1][1]
            assert 4 - 1e-12 <= w <= 5 + 1e-12 and 4 - 1e-12 <= h <= 10 + 1e-12
            assert 10 <= b[0][0] + w / 2 <= 30
        for d in s["dynamic"]:
            assert 0.2 <= d["rx"] <= 1.2 and 0.3 <= d["freq"] <= 0.7 and abs(d["p2"][0] - d["p1"][0]) <= 5
    m = rl_env.make_map(path=[s["start"][:2], s["goal"]], **s)      # the spec is make_map's keyword form
    assert len(m["obstacles"]) == 10


def test_pack_records_with_limits_keeps_the_layout_and_refuses_what_does_not_fit():
    from tests.support import env_maps
    rng = np.random.default_rng(3)
    maps = [env_maps.random_map(rng) for _ in range(6)]
    rec, maxima = rl_env.pack_records(maps)
    again, same = rl_env.pack_records(maps[2:4], limits=maxima)
    assert same == maxima and np.array_equal(again, rec[2:4])
    small = dict(maxima, n_edge_max=maxima["n_edge_max"] - 1)
    with pytest.raises(ValueError, match="n_edge_max"):
        rl_env.pack_records(maps, limits=small)


# ---- header and exports ------------------------------------------------------------------------------------------------------------
def test_plan_header_declares_the_exports_and_the_library_has_them():
    text = open(os.path.join(ROOT, "include", "mpcgpu_plan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mpcgpu_[a-z_0-9]+)\s*\(", text))
    assert declared == set(path_plan.PLAN_EXPORTS)
    path = solver_mod.library_path()
    assert os.path.exists(path), f"{path} missing -- run __graft_entry__.build()"
    lib = ctypes.CDLL(path)
    for sym in path_plan.PLAN_EXPORTS:
        assert hasattr(lib, sym), sym
    lib.mpcgpu_abi_version.restype = ctypes.c_int32
    assert lib.mpcgpu_abi_version() == 8
    assert not set(path_plan.PLAN_EXPORTS) & (set(solver_mod.EXPORTS) | set(rl_env.ENV_EXPORTS))
    # the limits are refused without a device
    lib.mpcgpu_plan_record_doubles.restype = ctypes.c_int32
    lib.mpcgpu_plan_last_error.restype = ctypes.c_char_p
    ok = path_plan._CPlanParams(256, 32, 64, 0)
    assert lib.mpcgpu_plan_record_doubles(ctypes.byref(ok)) == path_plan.record_doubles(256, 32) == 2 + 32 + 512
    for bad, word in ((path_plan._CPlanParams(257, 32, 64, 0), "256 ring vertices"), (path_plan._CPlanParams(256, 33, 64, 0), "32 rings"),
                      (path_plan._CPlanParams(256, 32, 65, 0), "64 path nodes")):
        assert lib.mpcgpu_plan_record_doubles(ctypes.byref(bad)) < 0
        assert word in lib.mpcgpu_plan_last_error().decode()
