"""GPU tests of map turnover on the image environment (``mpcgpu_env_step_imgs_fresh_dev``, include/mpcgpu_map.h): the fresh
image step against the pinned three-call form (step, replace_maps, reset) of the plain image kernels, bit for bit, and the
device map stream behind it.  The helpers are copies of those of tests/test_gpu_map_stream.py."""
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
B, LIMIT = 8, 12


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


def _img_env(maps, capacity, size, turnover, limit=LIMIT):
    return rl_env.BatchedImgsEnv(maps, max_episode_steps=limit, capacity=capacity, image_width=size[0], image_height=size[1],
                                 map_turnover=turnover)


# ---- 1, 2, 3. fresh image step == step, replace_maps, reset; rows without a spare; calls without auto-reset ----------------------------
@pytest.mark.parametrize("size", [(54, 54), (9, 11)], ids=["54x54", "9x11"])
def test_fresh_image_step_equals_step_replace_maps_reset(size):
    """Sixty steps of seeded random actions; rows 1, 5 and 6 turn over onto maps with other obstacle counts and sizes, the other
    rows reset on the map they have.  H W = 99 of the second size is no multiple of 4: the byte-store tail of the resize.

    The hazard this test must be able to see is a terminal image drawn from the record the row has MOVED TO.  For every row
    that turns over, a scratch environment on the new map is put at the terminal state (pose, clock) and observed: channel 0
    of that image has to differ from the terminal image the fresh step returned, for at least one of the three rows (with
    these spares and both sizes it does; the rows that differ are printed)."""
    import torch
    initial, spares, capacity = _maps()
    env = _img_env(initial, capacity, size, True)
    ctl = _img_env(initial, capacity, size, False)
    scratch = _img_env(list(spares.values()), capacity, size, False)
    slot = {b: i for i, b in enumerate(spares)}
    assert {k: getattr(env.params, k) for k in KEYS} == capacity
    assert env.obs_image.shape == (B, 3, size[1], size[0])
    env.enable_spares()
    _same(env.reset()["external"], ctl.reset()["external"], "reset")
    env.load_spares(list(spares), list(spares.values()))
    assert env.spare_ready.tolist() == [int(b in spares) for b in range(B)]
    pending = dict(spares)
    rng = np.random.default_rng(5)
    ends = np.zeros(B, dtype=int)
    hazard_visible = {}
    for t in range(60):
        acts = torch.from_numpy(rng.integers(0, 9, B))
        obs, rew, term, trunc, info = env.step(acts, auto_reset=True)
        cobs, crew, cterm, ctrunc, cinfo = ctl.step(acts)
        done = cterm | ctrunc
        end_flags = ctl.state[:, 7].clone()
        rows = [b for b in np.flatnonzero(done.cpu().numpy()) if b in pending]
        for b in rows:                                       # the terminal state on the NEW map: what a wrong record would give
            scratch.state[slot[b]] = ctl.state[b]
            wrong = scratch.observe()["external"][slot[b], 0]
            hazard_visible[int(b)] = not torch.equal(wrong, info["terminal_observation"]["external"][b, 0])
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
        # state[26]: flags of the last step, kept across an in-kernel reset; the three-call form overwrites it at the reset
        want = ctl.state.clone()
        want[:, 26] = torch.where(done, end_flags, want[:, 26])
        _same(env.state, want, (t, "state"))
        _same(env.img_state[:, :7], ctl.img_state[:, :7], (t, "img_state"))      # 8..15 are hand-over scratch
    print(f"{size}: episode ends {ends.tolist()}, terminal image differs from the new map's for rows {hazard_visible}")
    assert sorted(hazard_visible) == sorted(spares) and any(hazard_visible.values())
    assert ends.min() >= 4                                   # the step limit alone ends an episode every 12 steps
    loaded, stale = env.loaded.cpu().numpy(), env.stale.cpu().numpy()
    assert loaded.tolist() == [int(b in spares) for b in range(B)]
    # 2. rows without a spare reset on the map they have, counted in stale (their images were compared above)
    assert np.array_equal(stale, ends - loaded) and not pending
    assert all(stale[b] == ends[b] >= 4 for b in range(B) if b not in spares)
    assert env.which.tolist() == [int(b in spares) for b in range(B)] and env.spare_ready.tolist() == [0] * B
    _same(env.current_records(), ctl.records, "records")

    # 3. the calls without auto-reset act on the table a row is on
    for k in ("internal", "external"):
        _same(env.observe()[k], ctl.observe()[k], ("observe", k))
    acts = torch.from_numpy(rng.integers(0, 9, B))
    a, b_ = env.step(acts), ctl.step(acts)
    for k in ("internal", "external"):
        _same(a[0][k], b_[0][k], ("plain step", k))
    _same(env.state, ctl.state, "state after the plain step")
    _same(env.img_state[:, :7], ctl.img_state[:, :7], "img_state after the plain step")
    other = env_maps.random_map(np.random.default_rng(3), n_obst=(0, 2))
    env.replace_maps([5, 2], [other, other])
    ctl.replace_maps([5, 2], [other, other])
    mask = torch.tensor([False, True, True, False, False, True, False, False])
    before = (env.state.clone(), env.img_state.clone(), env.obs_internal.clone(), env.obs_image.clone(), env.reward.clone(),
              env.terminated.clone())
    eo, co = env.reset(mask), ctl.reset(mask)
    for k in ("internal", "external"):
        _same(eo[k], co[k], ("masked reset", k))
    _same(env.state, ctl.state, "state after the masked reset")
    _same(env.img_state[:, :7], ctl.img_state[:, :7], "img_state after the masked reset")
    _same(env.current_records(), ctl.records, "records after replace_maps")
    now = (env.state, env.img_state, env.obs_internal, env.obs_image, env.reward, env.terminated)
    for i, (x, y) in enumerate(zip(before, now)):
        _same(x[~mask.to(x.device)], y[~mask.to(x.device)], ("rows outside the mask", i))
    assert not torch.equal(before[3][mask.to(env.device)], env.obs_image[mask.to(env.device)])


# ---- 4. state_dict ---------------------------------------------------------------------------------------------------------------------
def test_state_dict_split_continues_bitwise():
    """A 40-step run split at step 20 into a freshly built environment on other initial maps: the spare of row 5 is loaded
    (step 19) and not yet used at the split, the one of row 3 is loaded later (step 26)."""
    import torch
    initial, spares, capacity = _maps()
    rng = np.random.default_rng(6)
    acts = torch.from_numpy(rng.integers(0, 9, (40, B)))

    def build(maps):
        env = _img_env(maps, capacity, (54, 54), True)
        env.enable_spares()
        return env

    def run(split):
        env = build(initial)
        env.reset()
        env.load_spares([1, 6], [spares[1], spares[6]])
        out = []
        for t in range(40):
            if t == 19:
                env.load_spares([5], [spares[5]])
            if t == 26:
                env.load_spares([3], [spares[1]])
            if t == split:
                saved = env.state_dict()
                assert {"records2", "which", "spare_ready", "loaded", "stale", "img_state", "obs_image"} <= set(saved)
                assert saved["records2"].shape == (2, B, env.records.shape[1])
                assert int(saved["spare_ready"][5]) == 1 and int(saved["loaded"][5]) == 0
                env = build(initial[::-1])                   # other maps: everything comes from the dict
                env.load_state_dict(saved)
            obs, rew, term, trunc, info = env.step(acts[t], auto_reset=True)
            out.append((obs["internal"], obs["external"], info["terminal_observation"]["external"], rew, term, trunc,
                        env.state.clone(), env.img_state[:, :7].clone(), env.which.clone(), env.spare_ready.clone(),
                        env.loaded.clone(), env.stale.clone()))
        return out, env

    whole, env_a = run(-1)
    parts, env_b = run(20)
    for t, (a, b) in enumerate(zip(whole, parts)):
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (t, i))
    _same(env_a.records2, env_b.records2, "tables")
    assert env_a.loaded.tolist() == [0, 1, 0, 1, 0, 1, 1, 0]
    plain = _img_env(initial, capacity, (54, 54), True)     # no enable_spares()
    with pytest.raises(ValueError):
        plain.load_state_dict(env_a.state_dict())
    with pytest.raises(ValueError):
        env_a.load_state_dict(plain.state_dict())


# ---- 5. the stream end to end ----------------------------------------------------------------------------------------------------------
def _layout(cap):
    P, M, K, E = (cap[k] for k in KEYS)
    an = 4 + (K + 1) + 3 * K
    o_edge = 16 + 4 * P + M * an
    R = o_edge + 5 * E
    return o_edge, E, R + (R & 1)


def _compare_records(dev, host, cap, tally):
    """Device record(s) against ``pack_records(make_map(...), limits=cap)``, by the rule of tests/test_gpu_map_stream.py: exact in
    front of the edge table, owners and padding; the float64 boundary within 1e-12 m; the obstacles' float32-rounded nodes equal
    or the ADJACENT float32 (counted in ``tally`` = [compared, adjacent]); float32 values below 2^-16 m within 1e-12 m."""
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


def _host_record(spec, nodes, cap):
    return rl_env.pack_records([rl_env.make_map(path=nodes, **spec)], limits=cap)[0][0]


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


def _stream_env(n=16, limit=10):
    env = rl_env.BatchedImgsEnv(_initial_maps(n), max_episode_steps=limit, capacity=map_stream.DYNAMIC_CAPACITY, map_turnover=True)
    env.enable_fresh_maps(seed=3, refill_every=2)
    return env


def test_stream_end_to_end():
    import torch
    path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
    N, STEPS = 16, 80
    acts = torch.from_numpy(np.random.default_rng(12).integers(0, 9, (STEPS, N)))

    def run(split=None):
        env = _stream_env(N)
        env.reset()
        nums, imgs = [], []
        for t in range(STEPS):
            if t == split:
                saved = env.state_dict()
                env = _stream_env(N)
                env.load_state_dict(saved)
            obs, rew, term, trunc, info = env.step(acts[t], auto_reset=True)
            nums.append(torch.cat([obs["internal"].double(), rew[:, None], term[:, None].double(), trunc[:, None].double(),
                                   env.state, env.img_state[:, :7], env.which[:, None].double(), env.loaded[:, None].double()], 1))
            imgs.append(torch.stack([obs["external"], info["terminal_observation"]["external"]]))
        return torch.stack(nums), torch.stack(imgs), env

    first, first_img, env = run()
    again, again_img, env2 = run()
    parts, parts_img, env3 = run(split=40)
    assert torch.equal(first, again) and torch.equal(first_img, again_img), "two environments with the same seed and actions differ"
    assert torch.equal(first, parts) and torch.equal(first_img, parts_img), "a run split by state_dict at step 40 differs"
    for e in (env2, env3):
        for k in ("records2", "which", "spare_ready", "loaded", "stale", "attempt"):
            assert torch.equal(getattr(env, k), getattr(e, k)), k
    loaded, attempt = env.loaded.cpu().numpy(), env.attempt.cpu().numpy()
    assert loaded.min() >= 1, loaded
    # every current record is the host-built record of one of the maps the row has drawn
    current = env.current_records().cpu().numpy()
    tally = [0, 0]
    for b in range(N):
        found = [n for n in range(attempt[b]) if map_stream.spec_of(3, b + N * n)["start"][1] == current[b, 6]]
        assert len(found) == 1, (b, found)
        spec = map_stream.spec_of(3, b + N * found[0])
        paths, status = path_plan.plan_reference_paths([spec])
        assert status[0] == 0
        _compare_records(current[b], _host_record(spec, paths[0], map_stream.DYNAMIC_CAPACITY), map_stream.DYNAMIC_CAPACITY, tally)
    print(f"stream: loaded {loaded.tolist()}, stale {env.stale.tolist()}, attempts {attempt.tolist()}, float32 values compared "
          f"{tally[0]}, adjacent {tally[1]}")
    assert tally[1] <= 1e-4 * tally[0]


# ---- 6. learner ------------------------------------------------------------------------------------------------------------------------
def test_learner_trains_on_fresh_image_maps():
    dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
    env = _stream_env(16)
    learner = dqn_train.DqnLearner(env, buffer_size=4096, learning_starts=0, batch_size=32)
    assert learner.image
    stats = learner.learn(16 * 60)
    assert stats["timesteps"] >= 16 * 60 and stats["episodes"] > 0
    assert int(env.loaded.sum()) > 0


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    initial, spares, capacity = _maps()
    img = rl_env.BatchedImgsEnv(initial[:2])
    with pytest.raises(NotImplementedError, match="map_turnover"):
        img.enable_spares()
    with pytest.raises(NotImplementedError, match="map_turnover"):
        img.enable_fresh_maps()
    assert img.records2 is None
    small = rl_env.BatchedImgsEnv(initial[:2], map_turnover=True)      # sized for its own maps: smaller than DYNAMIC_CAPACITY
    with pytest.raises(ValueError, match="DYNAMIC_CAPACITY"):
        small.enable_fresh_maps()
    assert small.records2 is None and not hasattr(small, "attempt")   # refused before anything was allocated
    with pytest.raises(rl_env.MpcGpuError):
        small.load_spares([0], [spares[5]])                  # no second table yet
    # an edge table whose staging does not fit the image kernel's LDS: refused at construction, with the library's text
    with pytest.raises(ValueError, match="too many outline edges"):
        rl_env.BatchedImgsEnv(initial[:2], capacity=dict(capacity, n_edge_max=2100), map_turnover=True)
