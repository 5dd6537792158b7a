"""The visibility-graph planner kernel (csrc/plangpu.hip) on the GPU: bitwise against its twin
(tests/support/plan_numpy.py) on the fixture, on seeded random maps and at its limits -- the largest graphs (N = 255), exact
ties between lanes, exact contacts, malformed records; batch independence; and ``BatchedRaysEnv.replace_maps`` /
``BatchedImgsEnv.replace_maps`` with planned maps."""
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import rl_env_numpy as orc
from tests.support import plan_maps
from tests.support import plan_numpy as twin
from trajtrack_mpcndqn_rlboost_amd import path_plan, rl_env

MpcGpuError = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver").MpcGpuError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planner():
    return path_plan.PathPlanner(device=0)


def plan_on_gpu(planner, maps):
    return planner.plan([m[0][0] for m in maps], [m[0][1:] for m in maps], [m[1] for m in maps], [m[2] for m in maps])


def assert_equals_twin(planner, maps):
    status, n_nodes, length, paths = plan_on_gpu(planner, maps)
    t_status, t_n, t_length, t_paths = twin.plan_batch([m[0] for m in maps], [m[1] for m in maps], [m[2] for m in maps])
    print("status counts (kernel):", np.bincount(status, minlength=5).tolist(), " (twin):", np.bincount(t_status, minlength=5).tolist())
    assert np.array_equal(status, t_status)
    assert np.array_equal(n_nodes, t_n)
    assert np.array_equal(length.view(np.int64), t_length.view(np.int64))
    for b, (p, q) in enumerate(zip(paths, t_paths)):
        assert np.array_equal(p, q), b
    return status, n_nodes, length, paths


def random_maps(seed, n):
    rng = np.random.default_rng(seed)
    return [plan_maps.spec_map(rl_env.random_dynamic_spec(rng)) for _ in range(n)]


# ---- kernel equals twin ---------------------------------------------------------------------------------------------------
def test_kernel_equals_twin_on_the_fixture(planner):
    _, maps, fx = plan_maps.fixture()
    status, n_nodes, length, paths = assert_equals_twin(planner, maps)
    assert np.array_equal(status, fx["twin_status"]) and np.array_equal(n_nodes, fx["twin_n_nodes"])
    assert np.array_equal(length, fx["twin_length"])
    for b, p in enumerate(paths):
        assert np.array_equal(p, fx["twin_nodes"][b, :n_nodes[b]])


def test_kernel_equals_twin_on_512_seeded_random_maps(planner):
    status, *_ = assert_equals_twin(planner, random_maps(11, 512))
    assert (status == 0).sum() >= 400


def test_kernel_equals_twin_at_the_limits(planner):
    maps = [plan_maps.many_vertices(256), plan_maps.comb_of_boxes(31), plan_maps.zigzag(62), plan_maps.zigzag(63)]
    assert sum(len(r) for r in maps[0][0]) == 256 and len(maps[1][0]) == 32
    status, n_nodes, _, _ = assert_equals_twin(planner, maps)
    assert status[2] == 0 and n_nodes[2] == 64
    assert status[3] == 3 and n_nodes[3] == 65
    assert status[0] == 0 and status[1] == 0


def test_analytic_cases_on_the_kernel(planner):
    room = [(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0)]
    sq = [(3.0, 2.0), (7.0, 2.0), (7.0, 6.0), (3.0, 6.0)]
    wall = [(4.0, -1.0), (6.0, -1.0), (6.0, 11.0), (4.0, 11.0)]
    cases = [(path_plan.oriented_rings(room, []), (1.0, 2.0), (9.0, 7.5)), (path_plan.oriented_rings(room, [sq]), (1.0, 1.0), (5.0, 4.0)),
             (path_plan.oriented_rings(room, [wall]), (1.0, 5.0), (9.0, 5.0)), (path_plan.oriented_rings(room, [sq]), (1.0, 1.0), (1.0, 1.0))]
    cases = [(r, np.asarray(s), np.asarray(g)) for r, s, g in cases]
    status, n_nodes, length, _ = assert_equals_twin(planner, cases)
    assert status.tolist() == [0, 2, 1, 0] and n_nodes.tolist() == [2, 0, 0, 2] and length[3] == 0.0


def test_a_257_vertex_map_is_refused_before_launch(planner):
    m = plan_maps.many_vertices(257)
    assert sum(len(r) for r in m[0]) == 257
    with pytest.raises(MpcGpuError, match="at most 256 ring vertices per map"):
        plan_on_gpu(planner, [m])
    with pytest.raises(MpcGpuError, match="at most 32 rings per map"):
        plan_on_gpu(planner, [plan_maps.comb_of_boxes(32)])
    torch.cuda.synchronize()


def test_a_malformed_record_is_status_4_and_touches_nothing_else(planner):
    """Good rows alternate with rows that are wrong in one way each.  Every wrong count is refused by a floating-point
    comparison before it is cast or used as an index (plangpu.hip, phase 1)."""
    maps = random_maps(5, 12)
    good, caps = path_plan.pack_rings([m[0] for m in maps])
    sg_good = np.array([np.concatenate([m[1], m[2]]) for m in maps])
    V, R = caps["n_vert_max"], caps["n_ring_max"]
    n_rings, n_vert = int(good[0, 0]), int(good[0, 1])
    assert n_rings >= 2 and n_vert >= 4
    # what is wrong -> {position in the record: value}; [0] ring count, [1] vertex count, [2 + k] size of ring k
    wrong = {"ring count 0": {0: 0.0}, "ring count n_ring_max + 1": {0: R + 1.0}, "ring count nan": {0: math.nan},
             "vertex count 2": {1: 2.0}, "vertex count nan": {1: math.nan},
             "a ring size of 2": {2: 2.0}, "a ring size of nan": {3: math.nan}, "a ring size of 1e300": {2: 1e300},
             "a ring size beyond the table": {2: 400.0},
             "ring sizes that are valid one by one and sum past n_vert_max": {1: V, **{2 + k: V for k in range(n_rings)}},
             "a vertex count that differs from the sum": {1: n_vert - 1.0}}
    rec, sg, kind = [], [], []                           # kind: the good map's number, or what is wrong
    for b, edits in zip(range(len(maps)), list(wrong.items()) + [None]):
        rec.append(good[b])
        sg.append(sg_good[b])
        kind.append(b)
        if edits is not None:
            bad = good[b].copy()
            for at, value in edits[1].items():
                bad[at] = value
            rec.append(bad)
            sg.append(sg_good[b])
            kind.append(edits[0])
    assert len(rec) == 12 + 11 and kind.count(0) == 1
    out = planner.plan_dev(torch.from_numpy(np.stack(rec)).cuda(), torch.from_numpy(np.stack(sg)).cuda(), **caps)
    status, n_nodes, nodes, length = (t.cpu().numpy() for t in out)
    for row, k in enumerate(kind):
        if isinstance(k, str):
            assert status[row] == 4 and n_nodes[row] == 0 and length[row] == 0.0 and not nodes[row].any(), k
            continue
        alone = planner.plan_dev(torch.from_numpy(good[k:k + 1].copy()).cuda(), torch.from_numpy(sg_good[k:k + 1].copy()).cuda(), **caps)
        a_status, a_n, a_nodes, a_length = (t.cpu().numpy() for t in alone)
        assert status[row] == a_status[0] == 0 and n_nodes[row] == a_n[0] >= 2, row
        assert np.array_equal(nodes[row], a_nodes[0]) and length[row:row + 1].view(np.int64) == a_length.view(np.int64), row


def test_batch_independence(planner):
    maps = random_maps(12, 511)
    _, fixture_maps, _ = plan_maps.fixture()
    probe = fixture_maps[4]
    alone = plan_on_gpu(planner, [probe])
    inside = plan_on_gpu(planner, maps[:300] + [probe] + maps[300:])
    assert len(inside[0]) == 512
    assert alone[0][0] == inside[0][300] == 0 and alone[1][0] == inside[1][300]
    assert alone[2][:1].view(np.int64) == inside[2][300:301].view(np.int64)
    assert np.array_equal(alone[3][0], inside[3][300])


# ---- the largest graphs, exact ties, exact contacts ----------------------------------------------------------------------------
def plan_rows(planner, maps, n_vert_max=None, n_ring_max=None):
    """One launch -> (status, n_nodes, nodes [B, 64, 2], length) as numpy, and the capacities used."""
    rec, caps = path_plan.pack_rings([m[0] for m in maps], n_vert_max, n_ring_max)
    sg = np.array([np.concatenate([m[1], m[2]]) for m in maps])
    out = planner.plan_dev(torch.from_numpy(rec).cuda(), torch.from_numpy(sg).cuda(), **caps)
    return tuple(t.cpu().numpy() for t in out), caps


def assert_rows_equal_recorded(got, rows, fx, where=None):
    """Rows ``rows`` of a launch against rows ``where`` (default: all, in order) of a recorded twin fixture, bit for bit."""
    status, n_nodes, nodes, length = got
    where = range(len(fx["twin_status"])) if where is None else where
    for row, i in zip(rows, where):
        assert status[row] == fx["twin_status"][i] and n_nodes[row] == fx["twin_n_nodes"][i], (row, i)
        assert length[row:row + 1].view(np.int64) == fx["twin_length"][i:i + 1].view(np.int64), (row, i)
        # all 128 doubles: the path where the status is 0, zeros behind it and in every other row
        assert np.array_equal(nodes[row], fx["twin_nodes"][i]), (row, i)
        if status[row] != 0:
            assert not nodes[row].any(), (row, i)


def test_all_limit_maps_in_one_launch_equal_the_recorded_twin(planner):
    """N = 255 (adjacency words 0 .. 7, four nodes per lane, compaction past rank 64), paths through graph index 251,
    NO_PATH after 121 settled nodes, the six ties -- with the 12 small fixture maps in between, so that a large graph's
    neighbours in the launch are small ones."""
    named, fx = plan_maps.limit_maps(), plan_maps.limits_fixture()
    _, small, small_fx = plan_maps.fixture()
    maps, big_rows, small_rows = [], [], []
    for i, (_, m) in enumerate(named):
        big_rows.append(len(maps))
        maps.append(m)
        if i < len(small):
            small_rows.append(len(maps))
            maps.append(small[i])
    got, caps = plan_rows(planner, maps)
    assert caps == dict(n_vert_max=256, n_ring_max=32) and len(small_rows) == 12
    print("status:", got[0].tolist())
    assert_rows_equal_recorded(got, big_rows, fx)
    assert_rows_equal_recorded(got, small_rows, small_fx)
    assert np.bincount(got[0][big_rows], minlength=5).tolist() == [15, 1, 1, 1, 0]


@pytest.mark.parametrize("name", ["saw_hall(60, 40)", "tie_square(7, 8, 7)"])
def test_tight_capacities_and_both_paddings_of_the_record(planner, name):
    """Alone at the tightest capacities, and with one ring more: the record is 2 + R + 2 V doubles padded to an even count
    and the coordinates start at 2 + n_ring_max, so one of the two is padded and the other is not."""
    named, fx = plan_maps.limit_maps(), plan_maps.limits_fixture()
    i = [n for n, _ in named].index(name)
    m = named[i][1]
    V, R = sum(len(r) for r in m[0]), len(m[0])
    lengths = []
    for n_ring_max in (R, R + 1):
        got, caps = plan_rows(planner, [m], n_ring_max=n_ring_max)
        assert caps == dict(n_vert_max=V, n_ring_max=n_ring_max)
        lengths.append(path_plan.record_doubles(V, n_ring_max))
        assert got[0][0] == 0
        assert_rows_equal_recorded(got, [0], fx, [i])
    assert lengths[0] == lengths[1] == 2 + R + 1 + 2 * V                          # R padded, R + 1 not


def test_n_node_max_on_both_sides_of_a_path(planner):
    fx = plan_maps.limits_fixture()
    saw = plan_maps.saw_hall(60, 40)
    i = fx["names"].tolist().index("saw_hall(60, 40)")
    assert fx["twin_n_nodes"][i] == 42
    got, _ = plan_rows(path_plan.PathPlanner(device=0, n_node_max=42), [saw])
    assert_rows_equal_recorded(got, [0], fx, [i])
    (status, n_nodes, nodes, length), _ = plan_rows(path_plan.PathPlanner(device=0, n_node_max=41), [saw])
    assert status[0] == 3 and n_nodes[0] == 42 and length[0] == 0.0 and not nodes[0].any()
    empty = (path_plan.oriented_rings(plan_maps.ROOM, []), np.array([1.0, 2.0]), np.array([9.0, 7.5]))
    one_bend = (path_plan.oriented_rings(plan_maps.ROOM, [plan_maps.box(3, 2, 7, 6)]), np.array([1.0, 1.0]), np.array([9.0, 8.0]))
    (status, n_nodes, nodes, length), _ = plan_rows(path_plan.PathPlanner(device=0, n_node_max=2), [empty, one_bend])
    assert status.tolist() == [0, 3] and n_nodes.tolist() == [2, 3]
    assert nodes[0, :2].tolist() == [[1.0, 2.0], [9.0, 7.5]] and length[0] == math.sqrt(8.0 * 8.0 + 5.5 * 5.5)
    assert not nodes[0, 2:].any() and not nodes[1].any() and length[1] == 0.0


def test_exact_contacts_on_the_kernel(planner):
    cases = plan_maps.contact_cases()
    status, n_nodes, length, paths = assert_equals_twin(planner, [c[1] for c in cases])
    for b, (name, _, want_status, want_nodes, want_length) in enumerate(cases):
        assert status[b] == want_status and np.array_equal(paths[b], want_nodes) and length[b] == want_length, name
        assert n_nodes[b] == len(want_nodes), name


def test_batch_independence_at_size(planner):
    """The largest graph alone and as row 300 of 512."""
    probe = plan_maps.field_of_polygons(3)
    maps = random_maps(12, 511)
    alone, _ = plan_rows(planner, [probe])
    inside, caps = plan_rows(planner, maps[:300] + [probe] + maps[300:])
    assert caps == dict(n_vert_max=256, n_ring_max=32) and len(inside[0]) == 512
    assert alone[0][0] == inside[0][300] == 0 and alone[1][0] == inside[1][300] == 3
    assert alone[3][:1].view(np.int64) == inside[3][300:301].view(np.int64)
    assert np.array_equal(alone[2][0], inside[2][300])
    assert max(plan_maps.graph_indices(probe[0], alone[2][0, 1:2])) >= 224


# ---- replace_maps -----------------------------------------------------------------------------------------------------------
def planned_maps(planner, seed, n):
    """``n`` environment maps of random_dynamic_spec with the kernel's paths (unplannable draws are drawn again)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        specs = [rl_env.random_dynamic_spec(rng) for _ in range(n)]
        paths, _ = path_plan.plan_reference_paths(specs, planner=planner)
        out += [rl_env.make_map(path=p, **s) for s, p in zip(specs, paths) if p is not None]
    return out[:n]


def n_edges(m):
    return len(m["boundary_padded"]) + sum(len(o["padded_nodes"]) for o in m["obstacles"])


def fitting(candidates, old, n):
    """The first ``n`` candidates that fit a record table built from ``old``: the generator fixes the obstacle and key-frame
    counts, but the path length and the number of outline edges (the round-padded ellipses) vary from draw to draw."""
    P, E = max(len(o["path"]) for o in old), max(n_edges(o) for o in old)
    out = [m for m in candidates if len(m["path"]) <= P and n_edges(m) <= E][:n]
    assert len(out) == n
    return out


def snapshot(env):
    return [t.clone() for t in (env.state, env.obs_internal, env.obs_image if hasattr(env, "obs_image") else env.obs_external,
                                env.reward, env.terminated)]


def rows_equal(a, b, rows):
    return all(torch.equal(x[rows], y[rows]) for x, y in zip(a, b))


def test_replace_maps_equals_a_fresh_environment_and_leaves_the_other_rows_alone(planner):
    B, rows, keep = 8, [1, 5, 6], [0, 2, 3, 4, 7]
    old = planned_maps(planner, 21, B)
    new = fitting(planned_maps(planner, 22, 32), old, 3)
    acts = torch.from_numpy(np.random.default_rng(4).integers(0, 9, (60, B))).cuda()
    env, control = rl_env.BatchedRaysEnv(old), rl_env.BatchedRaysEnv(old)
    for e in (env, control):
        e.reset()
        for t in range(10):
            e.step(acts[t])
    assert rows_equal(snapshot(env), snapshot(control), list(range(B)))
    env.replace_maps(rows, new)
    mask = torch.zeros(B, dtype=torch.bool)
    mask[rows] = True
    # the one-step observation memory (state[8:24]) survives a reset, as the reference's component keeps old_obs across
    # episodes: the fresh environment is handed the same memory before its reset
    mixed = list(old)
    for r, m in zip(rows, new):
        mixed[r] = m
    fresh = rl_env.BatchedRaysEnv(mixed)
    fresh.state[:, 8:24] = env.state[:, 8:24]
    first = env.reset(mask)
    first_fresh = fresh.reset()
    assert torch.equal(first["internal"][rows], first_fresh["internal"][rows])
    assert torch.equal(first["external"][rows], first_fresh["external"][rows])
    assert rows_equal(snapshot(env), snapshot(control), keep)            # reset(mask) + replace_maps left the others alone
    for t in range(10, 60):
        out, out_c, out_f = env.step(acts[t]), control.step(acts[t]), fresh.step(acts[t])
        assert rows_equal(snapshot(env), snapshot(fresh), rows), t
        assert rows_equal(snapshot(env), snapshot(control), keep), t
        for k in (1, 2, 3):                                              # reward, terminated, truncated
            assert torch.equal(out[k][rows], out_f[k][rows]) and torch.equal(out[k][keep], out_c[k][keep])
        for k in ("internal", "external"):
            assert torch.equal(out[0][k][rows], out_f[0][k][rows]) and torch.equal(out[0][k][keep], out_c[0][k][keep])
    assert not rows_equal(snapshot(env), snapshot(control), rows)         # the replaced rows did change


def test_oracle_tracks_the_kernel_on_a_planned_map(planner):
    m = planned_maps(planner, 31, 1)[0]
    env = rl_env.BatchedRaysEnv([m] * 4)
    o = orc.OracleRaysEnv(m)
    env.reset()
    for a in np.random.default_rng(6).integers(0, 9, 25):
        obs, rew, term, _, _ = env.step(torch.full((4,), int(a)))
        oo, orew, odone, _ = o.step(int(a))
        # the tolerances of __graft_entry__._smoke_environment
        assert np.abs(env.agent_state[0].cpu().numpy() - o.state).max() <= 1e-12
        assert np.abs(obs["external"][0].cpu().numpy() - oo["external"]).max() <= 2e-6
        assert np.abs(obs["internal"][0].cpu().numpy() - oo["internal"]).max() <= 1e-6
        assert abs(float(rew[0]) - orew) <= 1e-9 and bool(term[0]) == odone


def test_replace_maps_on_the_image_environment(planner):
    B, rows = 4, [0, 2]
    old = planned_maps(planner, 41, B)
    new = fitting(planned_maps(planner, 42, 32), old, 2)
    env = rl_env.BatchedImgsEnv(old)
    env.reset()
    env.replace_maps(rows, new)
    mask = torch.zeros(B, dtype=torch.bool)
    mask[rows] = True
    mixed = list(old)
    for r, m in zip(rows, new):
        mixed[r] = m
    fresh = rl_env.BatchedImgsEnv(mixed)
    fresh.state[:, 8:24] = env.state[:, 8:24]
    a, b = env.reset(mask), fresh.reset()
    assert a["external"].dtype == torch.uint8 and a["external"][rows].any()
    assert torch.equal(a["external"][rows], b["external"][rows]) and torch.equal(a["internal"][rows], b["internal"][rows])


def test_a_map_too_large_for_the_record_table_raises_and_leaves_it_unchanged(planner):
    old = planned_maps(planner, 51, 4)
    env = rl_env.BatchedRaysEnv(old)
    env.reset()
    records, start = env.records.clone(), env._start.clone()
    big = dict(planned_maps(planner, 52, 1)[0])
    big["path"] = np.stack([np.linspace(5.0, 35.0, env.params.n_path_max + 1), np.full(env.params.n_path_max + 1, 10.0)], axis=1)
    with pytest.raises(ValueError, match="n_path_max"):
        env.replace_maps([0, 1], [old[2], big])
    edges = dict(old[0])
    edges["obstacles"] = old[0]["obstacles"] + old[1]["obstacles"][:1]
    with pytest.raises(ValueError, match="n_obst_max"):
        env.replace_maps([3], [edges])
    assert torch.equal(env.records, records) and torch.equal(env._start, start)
