"""GPU tests of per-episode map turnover (include/mpcgpu_map.h): the device draw against its host twin, and the fresh-map
variant of the auto-reset step against the pinned three-call form (step, replace_maps, reset) of the existing kernels."""
import importlib
import json
import os

import numpy as np
import pytest

from support import env_maps  # noqa: E402

pytestmark = pytest.mark.gpu
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
map_stream = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.map_stream")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "env_rays_traces.npz")
KEYS = ("n_path_max", "n_obst_max", "n_kf_max", "n_edge_max")


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------------------
def test_device_draw_equals_spec_of_bitwise_and_skips_ready_rows():
    import torch
    B, seed = 256, 11
    dev = torch.device("cuda", 0)
    table = torch.full((B, map_stream.SPEC_DOUBLES), -7.0, dtype=torch.float64, device=dev)
    ready = torch.zeros(B, dtype=torch.int32, device=dev)
    attempt = torch.zeros(B, dtype=torch.int32, device=dev)
    map_stream.draw_specs_dev(table, ready, attempt, seed)
    want = map_stream.pack_specs([map_stream.spec_of(seed, b) for b in range(B)])
    got = table.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert np.array_equal(attempt.cpu().numpy(), np.ones(B, dtype=np.int32))
    # second launch: every other row has its spare and is skipped; the rest move on to serial b + B
    ready[::2] = 1
    map_stream.draw_specs_dev(table, ready, attempt, seed)
    want2 = want.copy()
    want2[1::2] = map_stream.pack_specs([map_stream.spec_of(seed, b + B) for b in range(1, B, 2)])
    got2 = table.cpu().numpy()
    assert got2.tobytes() == want2.tobytes()
    assert np.array_equal(attempt.cpu().numpy(), np.where(np.arange(B) % 2 == 0, 1, 2).astype(np.int32))
    assert np.array_equal(ready.cpu().numpy(), (np.arange(B) % 2 == 0).astype(np.int32))
    # another seed is another stream
    map_stream.draw_specs_dev(table, torch.zeros_like(ready), attempt, seed + 1)
    assert not np.array_equal(table.cpu().numpy()[:, 1], want[:, 1])


# ---- 2. rings and plan -----------------------------------------------------------------------------------------------------------------
def _fixture_specs():
    """The 12 planner fixture maps (reflex, collinear and bevelled corners) as make_map keywords; two of them with two
    made-up periodic obstacles each, which the planner must not see."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "planner_maps.npz"))
    specs = [dict(s, dynamic=[], start=list(s["start"])[:2] + [0.3, 0.0, 0.0]) for s in json.loads(bytes(fx["specs_json"]).decode())]
    for i in (2, 7):
        gx, gy = specs[i]["goal"][:2]
        specs[i]["dynamic"] = [dict(p1=(gx, gy), p2=(gx + 1.0, gy - 2.0), freq=0.4, rx=0.7, ry=0.3, angle=1.0),
                               dict(p1=(gx - 3.0, gy), p2=(gx, gy + 2.5), freq=0.65, rx=0.25, ry=1.1, angle=4.0)]
    # none of the fixture's corners is collinear to 1e-14: a hall and a box with a vertex in the middle of an edge
    specs.append(dict(boundary=[(0.0, 0.0), (10.0, 0.0), (20.0, 0.0), (20.0, 12.0), (0.0, 12.0)],
                      static=[[(8.0, 4.0), (8.0, 6.0), (8.0, 8.0), (12.0, 8.0), (12.0, 4.0)]], dynamic=[],
                      start=[2.0, 6.0, 0.0, 0.0, 0.0], goal=[18.0, 6.0]))
    return specs


@pytest.mark.parametrize("which", ["drawn", "fixture"])
def test_device_rings_and_paths_equal_the_host_pipeline_bitwise(which):
    import torch
    path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
    specs = [map_stream.spec_of(11, b) for b in range(256)] if which == "drawn" else _fixture_specs()
    B = len(specs)
    dev = torch.device("cuda", 0)
    # host: inflate, orient, pack -- into the capacities the device writes
    rec, caps = path_plan.pack_rings([path_plan.oriented_rings(*path_plan.inflate_spec(s)) for s in specs],
                                     n_vert_max=map_stream.VERT_MAX, n_ring_max=map_stream.RING_MAX)
    sg = np.stack([np.concatenate([np.asarray(s["start"], dtype=np.float64)[:2],
                                   np.asarray(s["goal"], dtype=np.float32).astype(np.float64)[:2]]) for s in specs])
    table = torch.from_numpy(map_stream.pack_specs(specs)).to(dev)
    ready = torch.zeros(B, dtype=torch.int32, device=dev)
    ready[3] = 1                                             # a skipped row
    rings, start_goal = map_stream.rings_dev(table, ready)
    got, got_sg = rings.cpu().numpy(), start_goal.cpu().numpy()
    live = np.arange(B) != 3
    assert got.shape == rec.shape and got[3, 0] == 0.0
    assert got[live].tobytes() == rec[live].tobytes(), np.argwhere(got[live] != rec[live])[:6]
    assert got_sg[live].tobytes() == sg[live].tobytes()
    planner = path_plan.PathPlanner()
    dev_out = planner.plan_dev(rings, start_goal, **caps)
    sg_host = sg.copy()
    host_out = planner.plan_dev(torch.from_numpy(rec).to(dev), torch.from_numpy(sg_host).to(dev), **caps)
    status = dev_out[0].cpu().numpy()
    assert status[3] == 4
    for name, d, h in zip(("status", "n_nodes", "nodes", "length"), dev_out, host_out):
        d, h = d.cpu().numpy()[live], h.cpu().numpy()[live]
        assert d.tobytes() == h.tobytes(), name
    if which == "drawn":
        assert (status[live] == 0).mean() > 0.9              # generate_map_dynamic draws are almost always plannable
    else:
        # a bevelled corner adds a vertex; the last spec's path bends around the box that has the collinear vertex
        assert (rec[:, 1] - np.array([sum(len(r) for r in [s["boundary"]] + s["static"]) for s in specs])).sum() >= 2
        assert status[-1] == 0 and dev_out[1][-1].item() == 4


# ---- 3. records ------------------------------------------------------------------------------------------------------------------------
SENTINEL = -123.0


def _layout(cap):
    P, M, K, E = (cap[k] for k in KEYS)
    an = 4 + (K + 1) + 3 * K
    o_edge = 16 + 4 * P + M * an
    R = o_edge + 5 * E
    return o_edge, E, R + (R & 1)


def _compare_records(dev, host, cap, tally):
    """Device record(s) against ``pack_records(make_map(...), limits=cap)``.  Exact: everything in front of the edge table
    (counts, goal, start, path nodes and lengths, animation blocks), the owner column, the padding.  Outline coordinates come
    after cos / sin / atan2 / acos / hypot: the float64 boundary within 1e-12 m (coordinates are below 64 m, an ulp is 7e-15; a
    wrong vertex is off by 1e-6 at the very least), the obstacles' float32-rounded nodes equal or the ADJACENT float32
    (counted in ``tally`` = [compared, adjacent]).

    One class of float32 values cannot be held to adjacency: body-frame coordinates whose exact value is 0 (an ellipse node on an
    axis, r cos(a) at a = pi / 2) are rounding residues of about 1e-16 m, and float32 keeps such a residue to 24 bits of ITSELF:
    host -6.2e-17 against device +1.6e-16 was the first MI355X run's only miss, 2.2e-16 m apart -- one ulp of the operands that
    cancelled -- and a dozen million float32 steps from each other.  Below 2^-16 m the float32 grid is finer than 1e-12 m, the pass
    through float32 coarsens nothing there, and the float64 bound applies: such values must lie within 1e-12 m."""
    o_edge, E, R = _layout(cap)
    dev, host = np.atleast_2d(dev), np.atleast_2d(host)
    assert dev.shape == host.shape and dev.shape[1] == R
    assert dev[:, :o_edge].tobytes() == host[:, :o_edge].tobytes(), np.argwhere(dev[:, :o_edge] != host[:, :o_edge])[:6]
    assert dev[:, o_edge + 5 * E:].tobytes() == host[:, o_edge + 5 * E:].tobytes()
    de, he = dev[:, o_edge:o_edge + 5 * E].reshape(len(dev), E, 5), host[:, o_edge:o_edge + 5 * E].reshape(len(dev), E, 5)
    assert np.array_equal(de[:, :, 4], he[:, :, 4])                                   # owners and the -2 padding
    pad = he[:, :, 4] == -2.0
    assert np.array_equal(de[pad], he[pad])
    wall = he[:, :, 4] == -1.0
    if wall.any():
        assert np.abs(de[wall][:, :4] - he[wall][:, :4]).max() <= 1e-12
    obst = he[:, :, 4] >= 0.0
    d32, h32 = de[obst][:, :4].astype(np.float32), he[obst][:, :4].astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), de[obst][:, :4])                    # the device values ARE float32 values
    tiny = np.abs(h32) < 2.0 ** -16
    assert np.abs(d32[tiny].astype(np.float64) - h32[tiny].astype(np.float64)).max(initial=0.0) <= 1e-12
    differ = (d32 != h32) & ~tiny
    assert np.array_equal(np.nextafter(h32[differ], d32[differ]), d32[differ])        # ... equal or adjacent
    tally[0] += d32.size
    tally[1] += int(differ.sum())


def _refill_once(specs, cap, which=None, ready=None):
    """rings, planner and record kernels on ``specs`` -> (records2 [2, B, R], status, spare_ready, planner output)."""
    import ctypes
    import torch
    path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
    dev = torch.device("cuda", 0)
    B = len(specs)
    params = rl_env._CParams(num_segments=8, corner_samples=3, time_step=0.2, **cap, **rl_env.ROBOT)
    table = torch.from_numpy(map_stream.pack_specs(specs)).to(dev)
    ready = torch.zeros(B, dtype=torch.int32, device=dev) if ready is None else ready.to(dev)
    which = torch.zeros(B, dtype=torch.int32, device=dev) if which is None else which.to(dev)
    records2 = torch.full((2, B, _layout(cap)[2]), SENTINEL, dtype=torch.float64, device=dev)
    rings, sg = map_stream.rings_dev(table, ready)
    plan = path_plan.PathPlanner().plan_dev(rings, sg, map_stream.VERT_MAX, map_stream.RING_MAX)
    status = torch.full((B,), -9, dtype=torch.int32, device=dev)
    map_stream.records_dev(params, table, plan[0], plan[1], plan[2], records2, which, ready, status)
    return records2.cpu().numpy(), status.cpu().numpy(), ready.cpu().numpy(), [t.cpu().numpy() for t in plan]


def _host_record(spec, nodes, cap):
    return rl_env.pack_records([rl_env.make_map(path=nodes, **spec)], limits=cap)[0][0]


@pytest.mark.parametrize("which_set", ["drawn", "fixture"])
def test_device_records_equal_pack_records(which_set):
    import torch
    if which_set == "drawn":
        specs = [map_stream.spec_of(11, b) for b in range(256)]
        box = np.asarray(specs[9]["static"][0])
        specs[9] = dict(specs[9], goal=[float(box[:, 0].mean()), float(box[:, 1].mean())])   # a goal inside a box: status 2
        cap = dict(map_stream.DYNAMIC_CAPACITY)
    else:
        specs = _fixture_specs()
        cap = dict(n_path_max=16, n_obst_max=8, n_kf_max=2, n_edge_max=400)
    B = len(specs)
    which = torch.from_numpy((np.arange(B) % 3 == 0).astype(np.int32))
    ready = torch.zeros(B, dtype=torch.int32)
    ready[5] = 1                                                                       # a row that has its spare: skipped
    rec2, status, ready_out, plan = _refill_once(specs, cap, which, ready)
    assert status[5] == -1 and ready_out[5] == 1
    if which_set == "drawn":
        assert status[9] == 2
    ok = np.flatnonzero(status == 0)
    assert len(ok) >= 0.9 * (B - 2) and set(np.unique(status)) <= {-1, 0, 1, 2}
    tally, edges = [0, 0], []
    for b in range(B):
        spare, current = rec2[1 - int(which[b]), b], rec2[int(which[b]), b]
        assert (current == SENTINEL).all()                                            # the record a row is on is never touched
        if status[b] != 0:
            assert (spare == SENTINEL).all() and (ready_out[b] == 0 or b == 5)        # nothing of the row was written
            continue
        assert ready_out[b] == 1
        nodes = plan[2][b, :plan[1][b]]
        _compare_records(spare, _host_record(specs[b], nodes, cap), cap, tally)
        edges.append(int(spare[2]))
    share = tally[1] / max(tally[0], 1)
    print(f"{which_set}: {len(ok)} records, edges {min(edges)}..{max(edges)}, float32 values compared {tally[0]}, "
          f"adjacent instead of equal {tally[1]} (share {share:.2e})")
    assert share <= 1e-4
    if which_set == "drawn":
        assert max(edges) <= map_stream.DYNAMIC_CAPACITY["n_edge_max"]
        # a table one edge too small for the largest map: status 5 for exactly the maps that do not fit, nothing written
        small = dict(cap, n_edge_max=max(edges) - 1)
        rec2s, status_s, ready_s, _ = _refill_once(specs, small)
        big = np.array([status[b] == 0 and int(rec2[1 - int(which[b]), b, 2]) == max(edges) for b in range(B)])
        assert big.any() and np.array_equal(status_s == 5, big)
        rest = ~big & (np.arange(B) != 5)                                             # (row 5 is not skipped in this launch)
        assert np.array_equal(status_s[rest], status[rest])
        for b in np.flatnonzero(big):
            assert (rec2s[:, b] == SENTINEL).all() and ready_s[b] == 0


# ---- 4. fresh step == step, replace_maps, reset ----------------------------------------------------------------------------------------
def _maps():
    """8 initial maps (the two fixture scenes and random halls) and 3 spares with other sizes; the capacity of all of them."""
    fx = np.load(GOLD)
    specs = json.loads(bytes(fx["specs_json"]).decode())
    scenes = [rl_env.make_map(sp["boundary"], sp["static"], sp["dynamic"], sp["start"], sp["goal"], sp["path"])
              for sp in specs.values()]
    rng = np.random.default_rng(21)
    initial = [scenes[0], scenes[1]] + [env_maps.random_map(rng) for _ in range(6)]
    spares = {1: env_maps.random_map(rng, n_obst=5), 5: scenes[0], 6: env_maps.random_map(rng, n_obst=(0, 2))}
    _, capacity = rl_env.pack_records(initial + list(spares.values()))
    return initial, spares, capacity


def _same(a, b, what):
    import torch
    assert a.dtype == b.dtype and torch.equal(a, b), (what, (a != b).nonzero()[:4].tolist())


def test_fresh_step_equals_step_replace_maps_reset():
    import torch
    initial, spares, capacity = _maps()
    B, LIMIT = 8, 12
    env = rl_env.BatchedRaysEnv(initial, max_episode_steps=LIMIT, capacity=capacity)
    ctl = rl_env.BatchedRaysEnv(initial, max_episode_steps=LIMIT, capacity=capacity)
    assert {k: getattr(env.params, k) for k in KEYS} == capacity
    env.enable_spares()
    _same(env.reset()["external"], ctl.reset()["external"], "reset")
    env.load_spares(list(spares), list(spares.values()))
    assert env.spare_ready.tolist() == [int(b in spares) for b in range(B)]
    pending = dict(spares)
    rng = np.random.default_rng(5)
    ends = np.zeros(B, dtype=int)
    for t in range(60):
        acts = torch.from_numpy(rng.integers(0, 9, B))
        obs, rew, term, trunc, info = env.step(acts, auto_reset=True)
        cobs, crew, cterm, ctrunc, cinfo = ctl.step(acts)
        done = cterm | ctrunc
        end_flags = ctl.state[:, 7].clone()
        rows = [b for b in np.flatnonzero(done.cpu().numpy()) if b in pending]
        ctl.replace_maps(rows, [pending.pop(b) for b in rows])
        after = ctl.reset(done) if bool(done.any()) else cobs
        ends += done.cpu().numpy()
        for k in ("internal", "external"):
            _same(obs[k], after[k], (t, k))
            _same(info["terminal_observation"][k], cobs[k], (t, "terminal", k))
        _same(rew, crew, (t, "reward"))
        _same(term, cterm, (t, "terminated"))
        _same(trunc, ctrunc, (t, "truncated"))
        _same(info["success"], cinfo["success"], (t, "success"))
        # state[26] is documented as "flags of the last step, kept across an in-kernel reset": the three-call form overwrites
        # it with the flags of the reset observation, so for rows that ended it is compared with the flags the step left
        want = ctl.state.clone()
        want[:, 26] = torch.where(done, end_flags, want[:, 26])
        _same(env.state, want, (t, "state"))
    assert ends.min() >= 4                                   # the step limit alone ends an episode every 12 steps
    loaded, stale = env.loaded.cpu().numpy(), env.stale.cpu().numpy()
    assert loaded.tolist() == [int(b in spares) for b in range(B)]
    assert np.array_equal(stale, ends - loaded) and not pending
    assert env.which.tolist() == [int(b in spares) for b in range(B)] and env.spare_ready.tolist() == [0] * B
    _same(env.current_records(), ctl.records, "records")
    # the calls without auto-reset act on the table a row is on
    for k in ("internal", "external"):
        _same(env.observe()[k], ctl.observe()[k], ("observe", k))
    acts = torch.from_numpy(rng.integers(0, 9, B))
    _same(env.step(acts)[0]["external"], ctl.step(acts)[0]["external"], "plain step")
    other = env_maps.random_map(np.random.default_rng(3), n_obst=(0, 2))
    env.replace_maps([5, 2], [other, other])
    ctl.replace_maps([5, 2], [other, other])
    mask = torch.tensor([False, True, True, False, False, True, False, False])
    for k in ("internal", "external"):
        _same(env.reset(mask)[k], ctl.reset(mask)[k], ("masked reset", k))
    _same(env.state, ctl.state, "state after the masked reset")
    _same(env.current_records(), ctl.records, "records after replace_maps")


def test_state_dict_carries_both_tables_and_the_row_vectors():
    """A run split by state_dict / load_state_dict in the middle -- with one spare loaded and not yet used -- continues bitwise."""
    import torch
    initial, spares, capacity = _maps()
    B, LIMIT = 8, 12
    rng = np.random.default_rng(6)
    acts = torch.from_numpy(rng.integers(0, 9, (40, B)))

    def run(split):
        env = rl_env.BatchedRaysEnv(initial, max_episode_steps=LIMIT, capacity=capacity)
        env.enable_spares()
        env.reset()
        env.load_spares([1, 6], [spares[1], spares[6]])
        out = []
        for t in range(40):
            if t == 17:
                env.load_spares([5], [spares[5]])
            if t == split:
                saved = env.state_dict()
                assert {"records2", "which", "spare_ready", "loaded", "stale"} <= set(saved) and saved["records2"].shape == (2, B, env.records.shape[1])
                env = rl_env.BatchedRaysEnv(initial[::-1], max_episode_steps=LIMIT, capacity=capacity)   # other maps: all from the dict
                env.enable_spares()
                env.load_state_dict(saved)
            obs, rew, term, trunc, info = env.step(acts[t], auto_reset=True)
            out.append((obs["internal"], obs["external"], rew, term, trunc, env.state.clone(), env.which.clone(),
                        env.spare_ready.clone(), env.loaded.clone(), env.stale.clone()))
        return out, env

    whole, env_a = run(-1)
    parts, env_b = run(20)
    for t, (a, b) in enumerate(zip(whole, parts)):
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (t, i))
    _same(env_a.records2, env_b.records2, "tables")
    assert env_a.loaded.tolist() == [0, 1, 0, 0, 0, 1, 1, 0]
    plain = rl_env.BatchedRaysEnv(initial, capacity=capacity)
    with pytest.raises(ValueError):
        plain.load_state_dict(env_a.state_dict())


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    initial, spares, capacity = _maps()
    _, own = rl_env.pack_records(initial[:2])
    env = rl_env.BatchedRaysEnv(initial[:2])                 # sized for its own two maps
    with pytest.raises(rl_env.MpcGpuError):
        env.load_spares([0], [spares[5]])                    # no second table yet
    env.enable_spares()
    ring = initial[0]["boundary_padded"]
    big = dict(initial[0], boundary_padded=env_maps._pad_to_edges(ring, len(ring) + own["n_edge_max"] + 1 - env_maps.n_edges(initial[0])))
    assert env_maps.n_edges(big) == own["n_edge_max"] + 1
    before = env.records2.clone()
    with pytest.raises(ValueError, match="n_edge_max"):
        env.load_spares([0, 1], [initial[0], big])
    assert env.spare_ready.tolist() == [0, 0] and bool((env.records2 == before).all())   # nothing was written
    with pytest.raises(ValueError):
        env.load_spares([0, 0], [initial[0], initial[0]])
    with pytest.raises(ValueError, match="n_path_max"):
        rl_env.BatchedRaysEnv(initial, capacity=dict(capacity, n_path_max=2))
    img = rl_env.BatchedImgsEnv(initial[:2])
    with pytest.raises(NotImplementedError):
        img.enable_spares()


# ---- 5. the stream end to end ----------------------------------------------------------------------------------------------------------
_INITIAL = {}


def _initial_maps(n):
    """``n`` plannable generate_map_dynamic maps (host-built, stream 99) for the environments to start on."""
    if n not in _INITIAL:
        path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
        specs = [map_stream.spec_of(99, b) for b in range(2 * n)]
        paths, status = path_plan.plan_reference_paths(specs)
        _INITIAL[n] = [rl_env.make_map(path=p, **s) for s, p, st in zip(specs, paths, status) if st == 0][:n]
        assert len(_INITIAL[n]) == n
    return _INITIAL[n]


def _stream_env(B=16, limit=10):
    env = rl_env.BatchedRaysEnv(_initial_maps(B), max_episode_steps=limit, capacity=map_stream.DYNAMIC_CAPACITY)
    env.enable_fresh_maps(seed=3, refill_every=2)
    return env


def test_stream_end_to_end():
    import torch
    path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
    B, STEPS = 16, 80
    acts = torch.from_numpy(np.random.default_rng(12).integers(0, 9, (STEPS, B)))

    def run(split=None):
        env = _stream_env(B)
        env.reset()
        out = []
        for t in range(STEPS):
            if t == split:
                saved = env.state_dict()
                env = _stream_env(B)
                env.load_state_dict(saved)
            obs, rew, term, trunc, info = env.step(acts[t], auto_reset=True)
            out.append(torch.cat([obs["internal"].double(), obs["external"].double(), rew[:, None], term[:, None].double(),
                                  trunc[:, None].double(), env.state, env.which[:, None].double(), env.loaded[:, None].double()], 1))
        return torch.stack(out), env

    first, env = run()
    again, env2 = run()
    parts, env3 = run(split=40)
    assert torch.equal(first, again), "two environments with the same seed and actions differ"
    assert torch.equal(first, parts), "a run split by state_dict / load_state_dict at step 40 differs"
    for e in (env2, env3):
        for k in ("records2", "which", "spare_ready", "loaded", "stale", "attempt"):
            assert torch.equal(getattr(env, k), getattr(e, k)), k
    loaded, attempt = env.loaded.cpu().numpy(), env.attempt.cpu().numpy()
    assert loaded.min() >= 1, loaded
    # every current record is the host-built record of one of the maps the row has drawn
    current = env.current_records().cpu().numpy()
    tally = [0, 0]
    for b in range(B):
        found = [n for n in range(attempt[b]) if map_stream.spec_of(3, b + B * n)["start"][1] == current[b, 6]]
        assert len(found) == 1, (b, found)
        spec = map_stream.spec_of(3, b + B * found[0])
        paths, status = path_plan.plan_reference_paths([spec])
        assert status[0] == 0
        _compare_records(current[b], _host_record(spec, paths[0], map_stream.DYNAMIC_CAPACITY), map_stream.DYNAMIC_CAPACITY, tally)
    print(f"stream: loaded {loaded.tolist()}, stale {env.stale.tolist()}, attempts {attempt.tolist()}, float32 values compared "
          f"{tally[0]}, adjacent {tally[1]}")
    assert tally[1] <= 1e-4 * tally[0]


# ---- 6. learner ------------------------------------------------------------------------------------------------------------------------
def test_learner_trains_on_fresh_maps():
    dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
    env = _stream_env(16)
    learner = dqn_train.DqnLearner(env, buffer_size=4096, learning_starts=0, batch_size=32)
    stats = learner.learn(16 * 60)
    assert stats["timesteps"] >= 16 * 60 and stats["episodes"] > 0
    assert int(env.loaded.sum()) > 0


def test_fresh_maps_refusals():
    img = rl_env.BatchedImgsEnv(_initial_maps(16)[:2])
    with pytest.raises(NotImplementedError):
        img.enable_fresh_maps()
    env = rl_env.BatchedRaysEnv(_initial_maps(16)[:2])       # sized for its own maps: smaller than DYNAMIC_CAPACITY
    with pytest.raises(ValueError, match="DYNAMIC_CAPACITY"):
        env.enable_fresh_maps()
    assert env.records2 is None and not hasattr(env, "attempt")   # refused before anything was allocated
