"""Collection inside one launch on the GPU (include/mpcgpu_collect.h).

The action entry against its numpy twin, bit for bit; the defining property -- a launch of T steps equals T rounds of
``collect.act`` -> ``env.step(auto_reset=True)`` -> ``ReplayBuffer.add`` and the episode bookkeeping of ``DqnLearner.learn``, in
every bit of the environment's tensors, the ring, the episode returns and the [T, B] outputs --; split launches, the ring
wrapping inside a launch, untouched rows, NULL outputs, graph replay, refusals; and ``DqnLearner(collect_in_kernel=True)``.

Environments: tests/support/collect_cases.py (``max_episode_steps = 3``; row kinds that run into the time limit, end at once and
end later).  Every run with at least five rows asserts, from its [T, B] outputs, that it held a termination, a truncation, an
explored and a greedy action; a run of ONE row is a time-limit row and holds no termination."""
import numpy as np
import pytest
import torch

from support import collect_cases as cc, collect_numpy as cn, dqn_cases, dqn_numpy as tw
from trajtrack_mpcndqn_rlboost_amd import collect, dqn_train, rl_env
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
ENV_TENSORS = ("state", "obs_internal", "obs_external", "reward", "terminated", "truncated", "term_internal", "term_external")
OUT_NAMES = tuple(name for name, _ in collect.OUTPUTS)
SEED = 0x5EED_0000_0000_0001


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def theta_of(seed=3) -> torch.Tensor:
    return torch.from_numpy(dqn_cases.random_theta(np.random.default_rng(seed))).to(DEV)


def make_env(B, lead=2):
    """The environment of ``cc.maps(B)`` after a reset and ``lead`` host-driven steps (the time-limit rows are then one step
    from their limit, so a launch of one step holds a truncation)."""
    env = rl_env.BatchedRaysEnv(cc.maps(B), max_episode_steps=cc.MAX_EPISODE_STEPS)
    env.reset()
    for k in range(lead):
        env.step(torch.full((B,), 4 if k else 1, dtype=torch.int32), auto_reset=True)
    return env


def make_buffer(capacity, pos=0, size=0, per=False):
    buf = dqn_train.ReplayBuffer(capacity, 46, torch.device(DEV), per_kwargs={} if per else None)
    g = torch.Generator().manual_seed(capacity)
    for name in buf.FIELDS:                                  # rows no launch wrote keep these values
        x = getattr(buf, name)
        x.copy_((torch.rand(x.shape, generator=g) * 100 + 7).to(x.dtype))
    buf.pos, buf.size = pos, size
    return buf


def new_out(T, B):
    return {name: torch.zeros(T, B, dtype=dtype, device=DEV) for name, dtype in collect.OUTPUTS}


def host_rounds(env, theta, buf, eps, seed, serial, ep_return, out):
    """T rounds of the public single-step pieces, with the bookkeeping of ``DqnLearner.learn``."""
    for t, e in enumerate(eps):
        obs = dqn_train.flatten_observation(env._obs())
        actions = collect.act(env, theta, e, seed, serial + t)
        nxt, reward, terminated, truncated, info = env.step(actions, auto_reset=True)
        done = terminated | truncated
        buf.add(obs, dqn_train.flatten_observation(info["terminal_observation"]), actions, reward, terminated)
        ep_return += reward
        out["actions"][t], out["done"][t], out["success"][t] = actions, done.to(torch.uint8), info["success"].to(torch.uint8)
        out["episode_return"][t] = torch.where(done, ep_return, out["episode_return"][t])
        ep_return.copy_(torch.where(done, torch.zeros_like(ep_return), ep_return))


def snapshot(env, buf, ep_return, out=None):
    d = {"env." + k: getattr(env, k).clone() for k in ENV_TENSORS}
    d.update({"buf." + k: getattr(buf, k).clone() for k in buf.FIELDS})
    d["ep_return"] = ep_return.clone()
    d["pos_size"] = torch.tensor([buf.pos, buf.size])
    if out is not None:
        d.update({"out." + k: v.clone() for k, v in out.items()})
    return d


def restore(snap, env, buf, ep_return):
    for k in ENV_TENSORS:
        getattr(env, k).copy_(snap["env." + k])
    for k in buf.FIELDS:
        getattr(buf, k).copy_(snap["buf." + k])
    ep_return.copy_(snap["ep_return"])
    buf.pos, buf.size = (int(v) for v in snap["pos_size"])


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not same_bits(a[k], b[k])]


def run_pair(B, T, capacity=None, pos0=0, size0=0, eps=None, serial=5, with_out=True, lead=2, theta=None):
    """The launch and the T host rounds from the same start -> (launch snapshot, host snapshot, launch outputs, eps)."""
    eps = cc.mixed_eps(T) if eps is None else eps
    theta = theta_of() if theta is None else theta
    capacity = capacity or T * B + 11
    snaps = []
    for launch in (True, False):
        env, buf = make_env(B, lead), make_buffer(capacity, pos0, size0)
        ep = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device=DEV)
        out = new_out(T, B)
        if launch:
            collect.collect_rays(env, theta, buf, eps, SEED, serial, ep, out if with_out else None)
            kept = out
        else:
            host_rounds(env, theta, buf, eps, SEED, serial, ep, out)
        snaps.append(snapshot(env, buf, ep, out if (with_out or not launch) else None))
    return snaps[0], snaps[1], kept, eps


def assert_census(host, eps, serial, B):
    """From the [T, B] outputs of a run (``host``: the snapshot that has them): all four kinds of transitions when B >= 5."""
    done = host["out.done"].cpu().numpy().astype(bool)
    T = done.shape[0]
    ring_dones = host["buf.dones"]
    explored = np.array([[cn.uniform_of(cn.draw_bits(SEED, serial + t, b)[0]) < eps[t] for b in range(B)] for t in range(T)])
    kinds = np.arange(B) % 3
    truncations = int(done[:, kinds == 0].sum())
    terminations = int(done[:, kinds != 0].sum())
    print(f"B {B} T {T}: terminations {terminations}, truncations {truncations}, explored {int(explored.sum())}, "
          f"greedy {int((~explored).sum())}, successes {int(host['out.success'].sum())}")
    if B >= 5:
        assert terminations >= 1 and truncations >= 1 and explored.any() and (~explored).any()
        assert float(ring_dones.sum()) >= 1.0
    else:
        assert truncations >= 1 and terminations == 0        # the one row is a time-limit row, one step from its limit
    return explored


# ---- the action entry against the twin ---------------------------------------------------------------------------------------
def tie_thetas():
    rng = np.random.default_rng(21)
    tied = dqn_cases.random_theta(rng)
    W2, b2 = tw.split(tied)[4:]
    W2[7] = W2[3]
    b2[:] = 0.0
    b2[[3, 7]] = 50.0
    return {"random": dqn_cases.random_theta(rng), "zero": np.zeros(tw.NP, F), "tied_3_7": tied}


@pytest.mark.parametrize("B", [1, 9, 64, 257])
def test_act_equals_the_twin_bit_for_bit(B):
    rng = np.random.default_rng(B)
    x = rng.uniform(-1.0, 1.0, (B, 46)).astype(F)
    obs = {"external": torch.from_numpy(x[:, :32].copy()).to(DEV), "internal": torch.from_numpy(x[:, 32:].copy()).to(DEV)}
    for name, theta in tie_thetas().items():
        th = torch.from_numpy(theta).to(DEV)
        for eps in (0.0, 0.3, 1.0):
            for serial in (0, 2 ** 40):
                a, q = collect.act(obs, th, eps, SEED, serial, return_q=True)
                want_a, want_q, explored, _ = cn.act(theta, x, eps, SEED, serial)
                assert np.array_equal(q.cpu().numpy().view(np.uint32), want_q.view(np.uint32)), (name, eps, serial)
                assert np.array_equal(a.cpu().numpy(), want_a), (name, eps, serial)
                if eps == 0.0:
                    assert not explored.any()
                    if name == "zero":
                        assert not a.any()
                    if name == "tied_3_7":
                        assert (a == 3).all()
                if eps == 1.0:
                    assert explored.all()
    # the flat tensor and the environment's own observation are the same rows
    flat = torch.from_numpy(x).to(DEV)
    th = torch.from_numpy(tie_thetas()["random"]).to(DEV)
    assert torch.equal(collect.act(flat, th, 0.3, SEED, 7), collect.act(obs, th, 0.3, SEED, 7))


def test_act_on_the_environment_reads_the_observation_it_holds():
    env, th = make_env(9), theta_of()
    x = cn.flat(env.obs_external.cpu().numpy(), env.obs_internal.cpu().numpy())
    a, q = collect.act(env, th, 0.3, SEED, 3, return_q=True)
    want_a, want_q, explored, _ = cn.act(th.cpu().numpy(), x, 0.3, SEED, 3)
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(q.cpu().numpy().view(np.uint32), want_q.view(np.uint32))


# ---- the defining property ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("T", [1, 2, 7, 64])
def test_a_launch_of_t_steps_equals_t_host_rounds(B, T):
    serial = 5
    if T == 1:      # one step: an epsilon of 0.37, and the first serial at which the rows split into explored and greedy (exact, on the CPU)
        eps = [0.37]
        while B >= 5 and len({cn.uniform_of(cn.draw_bits(SEED, serial, b)[0]) < 0.37 for b in range(B)}) < 2:
            serial += 1
    else:
        eps = cc.mixed_eps(T)
    launch, host, out, eps = run_pair(B, T, eps=eps, serial=serial)
    assert differing(launch, host) == []
    assert_census(host, eps, serial, B)
    assert tuple(int(v) for v in launch["pos_size"]) == ((T * B) % (T * B + 11), T * B)
    # rows outside the written range keep what they held
    untouched = make_buffer(T * B + 11)
    for k in untouched.FIELDS:
        assert same_bits(launch["buf." + k][T * B:], getattr(untouched, k)[T * B:]), k
        assert not same_bits(launch["buf." + k][:T * B], getattr(untouched, k)[:T * B]), k


def test_every_step_leaves_the_reward_of_a_launch_of_its_own_in_double():
    """The ring keeps rewards as float32 and an episode return is a sum; here 40 launches of one step and 40 host rounds are
    compared after EVERY step, so a reward (float64, never fed back into the state) that rounds differently shows where it arises."""
    B, steps, theta = 64, 40, theta_of()
    envs, bufs = [make_env(B), make_env(B)], [make_buffer(steps * B), make_buffer(steps * B)]
    eps_ret = [torch.zeros(B, dtype=torch.float64, device=DEV) for _ in range(2)]
    outs = [new_out(1, B), new_out(1, B)]
    for t in range(steps):
        eps = [cc.mixed_eps(steps)[t]]
        collect.collect_rays(envs[0], theta, bufs[0], eps, SEED, 100 + t, eps_ret[0], outs[0])
        host_rounds(envs[1], theta, bufs[1], eps, SEED, 100 + t, eps_ret[1], outs[1])
        assert differing(snapshot(envs[0], bufs[0], eps_ret[0], outs[0]), snapshot(envs[1], bufs[1], eps_ret[1], outs[1])) == [], t
        for o in outs:
            o["episode_return"].zero_()
    assert float(bufs[0].dones.sum()) > 10


def test_split_launches_equal_one_launch():
    B, T, serial = 5, 7, 9
    eps, theta = cc.mixed_eps(T), theta_of()
    whole, _, _, _ = run_pair(B, T, eps=eps, serial=serial)
    env, buf = make_env(B), make_buffer(T * B + 11)
    ep, out = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device=DEV), new_out(T, B)
    collect.collect_rays(env, theta, buf, eps[:3], SEED, serial, ep, {k: v[:3] for k, v in out.items()})
    assert (buf.pos, buf.size) == (3 * B, 3 * B)
    collect.collect_rays(env, theta, buf, eps[3:], SEED, serial + 3, ep, {k: v[3:] for k, v in out.items()})
    assert differing(whole, snapshot(env, buf, ep, out)) == []


def test_the_ring_wraps_inside_a_launch():
    B, T = 5, 7
    capacity = T * B
    launch, host, out, eps = run_pair(B, T, capacity=capacity, pos0=capacity - B - 1, size0=capacity - B - 1)
    assert differing(launch, host) == []
    assert tuple(int(v) for v in launch["pos_size"]) == (capacity - B - 1, capacity)
    fresh = make_buffer(capacity)
    assert not (launch["buf.obs"] == fresh.obs).all(dim=1).any()            # T * B = capacity: every row was written
    # row (pos0 + t B + b) mod capacity holds the action of (t, b)
    rows = (capacity - B - 1 + torch.arange(T * B, device=DEV)) % capacity
    assert torch.equal(launch["buf.actions"][rows], out["actions"].reshape(-1).to(torch.int64))
    assert_census(host, eps, 5, B)


def test_null_outputs_change_nothing_else():
    with_out, host, _, _ = run_pair(5, 7)
    without, _, _, _ = run_pair(5, 7, with_out=False)
    assert differing(without, {k: v for k, v in with_out.items() if not k.startswith("out.")}) == []
    assert differing(with_out, host) == []


def test_a_captured_launch_replays_to_the_same_bits():
    B, T, serial = 5, 7, 5
    eps, theta = cc.mixed_eps(T), theta_of()
    env, buf = make_env(B), make_buffer(T * B + 11)
    ep, out = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device=DEV), new_out(T, B)
    start = snapshot(env, buf, ep)
    collect.collect_rays(env, theta, buf, eps, SEED, serial, ep, out)
    want = snapshot(env, buf, ep, out)
    restore(start, env, buf, ep)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        collect.collect_rays(env, theta, buf, eps, SEED, serial, ep, out)
    for _ in range(2):
        restore(start, env, buf, ep)
        for v in out.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        buf.pos, buf.size = (int(v) for v in want["pos_size"])
        assert differing(snapshot(env, buf, ep, out), want) == []


def test_refusals_leave_everything_as_it_was():
    B, T = 5, 4
    env, buf, theta = make_env(B), make_buffer(T * B + 3, pos=2, size=2), theta_of()
    ep = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device=DEV)
    out = new_out(T, B)
    before = snapshot(env, buf, ep, out)
    nan = float("nan")
    for eps, text in (([0.5] * 65, "1 <= T <= 64"), ([], "1 <= T <= 64"), ([0.5] * 5, "T * B must not exceed capacity"),
                      ([0.5, 0.5, 1.5, 0.5], "must lie in [0, 1]"), ([0.5, nan, 0.5, 0.5], "must lie in [0, 1]"),
                      ([-0.1, 0.5, 0.5, 0.5], "must lie in [0, 1]")):
        o = None if len(eps) != T else out
        with pytest.raises(MpcGpuError, match=text.replace("[", r"\[").replace("]", r"\]").replace("*", r"\*")):
            collect.collect_rays(env, theta, buf, eps, SEED, 0, ep, o)
    env.max_episode_steps = 0
    with pytest.raises(MpcGpuError, match="max_episode_steps must be positive"):
        collect.collect_rays(env, theta, buf, [0.5] * T, SEED, 0, ep, out)
    env.max_episode_steps = cc.MAX_EPISODE_STEPS
    with pytest.raises(ValueError, match="theta"):
        collect.collect_rays(env, theta[:100], buf, [0.5] * T, SEED, 0, ep, out)
    with pytest.raises(ValueError, match="ep_return"):
        collect.collect_rays(env, theta, buf, [0.5] * T, SEED, 0, ep.float(), out)
    torch.cuda.synchronize()
    assert differing(snapshot(env, buf, ep, out), before) == []
    spares = make_env(3)
    spares.enable_spares()
    with pytest.raises(ValueError, match="enable_spares"):
        collect.collect_rays(spares, theta, make_buffer(64), [0.5], SEED, 0, torch.zeros(3, dtype=torch.float64, device=DEV))


def test_each_step_reads_its_own_epsilon():
    """Only eps of step 3 of 7 changes, from 0.2 to 0.8: up to that step the two launches are the same, and at step 3 exactly the
    rows whose u lies in [0.2, 0.8) leave their greedy action for their random draw."""
    B, T, serial, lo, hi = 64, 7, 11, 0.2, 0.8
    eps = [0.5, 0.1, 0.9, lo, 0.5, 0.5, 0.5]
    a, _, out_a, _ = run_pair(B, T, eps=eps, serial=serial)
    b, _, out_b, _ = run_pair(B, T, eps=eps[:3] + [hi] + eps[4:], serial=serial)
    act_a, act_b = out_a["actions"].cpu().numpy(), out_b["actions"].cpu().numpy()
    assert np.array_equal(act_a[:3], act_b[:3])
    draws = [cn.draw_bits(SEED, serial + 3, r) for r in range(B)]
    u = np.array([cn.uniform_of(e) for e, _ in draws])
    rnd = np.array([cn.random_of(x) for _, x in draws])
    band = (u >= lo) & (u < hi)
    assert 10 <= band.sum() <= B - 10
    assert np.array_equal(act_b[3][band], rnd[band])                      # explored under 0.8 ...
    assert np.array_equal(act_a[3][u < lo], rnd[u < lo])                  # ... as the rows below 0.2 are in both
    assert np.array_equal(act_a[3] != act_b[3], band & (rnd != act_a[3]))   # greedy under 0.2: changed unless the draw is the greedy action
    assert (act_a[3] != act_b[3]).sum() >= 5


# ---- the learner -----------------------------------------------------------------------------------------------------------
def learner(launch_steps, B=8, **kw):
    torch.manual_seed(1)
    env = rl_env.BatchedRaysEnv(cc.maps(B), max_episode_steps=cc.MAX_EPISODE_STEPS)
    kw.setdefault("fused", True)
    return dqn_train.DqnLearner(env, buffer_size=256, learning_starts=24, batch_size=16, train_freq=4, gradient_steps=2,
                                target_update_interval=40, seed=4, collect_in_kernel=True, collect_launch_steps=launch_steps, **kw)


def flat_items(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from flat_items(v, f"{prefix}{k}.")
        else:
            yield prefix + str(k), v


def assert_same_checkpoint(a, b):
    a, b = dict(flat_items(a)), dict(flat_items(b))
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert same_bits(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


@pytest.mark.parametrize("setting", [dict(), dict(per=True, per_in_kernel=True)], ids=["fused", "fused_per_in_kernel"])
def test_learner_step_by_step_launches_equal_whole_rounds(setting):
    one, whole = learner(1, **setting), learner(None, **setting)
    stats_one, stats_whole = one.learn(200), whole.learn(200)
    assert stats_one.keys() == stats_whole.keys()
    assert all(stats_one[k] == stats_whole[k] or (stats_one[k] != stats_one[k] and stats_whole[k] != stats_whole[k]) for k in stats_one)
    assert stats_one["timesteps"] == 200 and stats_one["updates"] > 0 and stats_one["episodes"] > 20
    assert one.episode_returns == whole.episode_returns and one.episode_successes == whole.episode_successes
    assert len(one.episode_returns) == stats_one["episodes"] and any(one.episode_successes)
    assert_same_checkpoint(one.state_dict(), whole.state_dict())
    assert one.collect_serial == whole.collect_serial == 25 and one.n_calls == 25 and one.trainer.num_target_syncs == whole.trainer.num_target_syncs >= 4
    assert one.buffer.size == 200 and one.buffer.pos == 200
    if setting:
        assert same_bits(one.buffer.sum_tree.tree, whole.buffer.sum_tree.tree) and same_bits(one.buffer.sum_tree.state, whole.buffer.sum_tree.state)
        assert len(set(one.buffer.sum_tree.tree.cpu().tolist())) > 3
    # the device counters of track_episodes=False are formed per step: the same bits as the lists' sums, step by step
    counted = learner(None, track_episodes=False, **setting)
    stats = counted.learn(200)
    assert stats["episodes"] == stats_whole["episodes"] == int(counted.ep_count)
    assert int(counted.ep_success_sum) == sum(whole.episode_successes)
    # (another order of the same float64 additions: some 75 terms of magnitude 1, so 1e-9 is generous)
    assert abs(float(counted.ep_return_sum) - sum(whole.episode_returns)) <= 1e-9 * max(1.0, abs(sum(whole.episode_returns)))
    counted_one = learner(1, track_episodes=False, **setting)
    counted_one.learn(200)
    assert_same_checkpoint(counted_one.state_dict(), counted.state_dict())


def test_learner_continues_from_a_checkpoint_to_the_same_end(tmp_path):
    whole = learner(None)
    whole.learn(200)
    first = learner(None)
    first.learn(200, stop_at=96)
    assert first.num_timesteps == 96
    first.save(str(tmp_path / "ck.pt"))
    second = learner(None)
    second.collect_seed = 0                     # the checkpoint brings its own
    second.load(str(tmp_path / "ck.pt"))
    assert (second.collect_seed, second.collect_serial) == (whole.collect_seed, 12)
    second.learn(200)
    assert_same_checkpoint(second.state_dict(), whole.state_dict())


def test_learner_with_the_plain_trainer_fills_the_buffer():
    lr = learner(None, fused=False)
    assert isinstance(lr.trainer, dqn_train.DqnTrainer)
    before = [p.detach().clone() for p in lr.trainer.q_net.parameters()]
    stats = lr.learn(200)
    assert stats["timesteps"] == 200 and stats["updates"] > 0 and np.isfinite(stats["loss"])
    assert lr.buffer.size == 200 and lr.collect_serial == 25
    assert int(lr.buffer.actions[:200].min()) >= 0 and int(lr.buffer.actions[:200].max()) <= 8 and len(set(lr.buffer.actions[:200].tolist())) > 3
    assert bool(lr.buffer.obs[:200].abs().sum(dim=1).gt(0).all()) and float(lr.buffer.dones[:200].sum()) > 0
    assert any(not torch.equal(p, q) for p, q in zip(lr.trainer.q_net.parameters(), before))
