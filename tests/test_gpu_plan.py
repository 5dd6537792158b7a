"""The visibility-graph planner kernel (csrc/plangpu.hip) on the GPU: bitwise against its twin
(tests/support/plan_numpy.py) on the fixture, on seeded random maps and at its limits; batch independence; and
``BatchedRaysEnv.replace_maps`` / ``BatchedImgsEnv.replace_maps`` with planned maps."""
import importlib

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
    maps = random_maps(5, 3)
    rec, caps = path_plan.pack_rings([m[0] for m in maps])
    rec[1, 2] = 400.0                                    # a ring size beyond the table
    sg = np.array([np.concatenate([m[1], m[2]]) for m in maps])
    status, n_nodes, nodes, length = planner.plan_dev(torch.from_numpy(rec).cuda(), torch.from_numpy(sg).cuda(), **caps)
    good = plan_on_gpu(planner, maps)
    assert status.cpu().tolist() == [int(good[0][0]), 4, int(good[0][2])]
    assert n_nodes[1].item() == 0 and not nodes[1].any().item() and length[1].item() == 0.0
    assert np.array_equal(length.cpu().numpy()[[0, 2]], good[2][[0, 2]])


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
