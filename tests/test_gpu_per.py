"""GPU tests of prioritized experience replay: the HIP sum tree (csrc/pergpu.hip through per_tree.SumTree) against its numpy
twin (tests/support/per_numpy.py) -- tree (leaves included: the device restates the C library's pow), indices and state
block bitwise, weights to one float32 ulp -- and ``DqnLearner(per=True)`` on both environments.  None of this exists without the feature: no
``mpcgpu_per_*`` symbols, no ``per=`` argument."""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from support import per_numpy  # noqa: E402

pytestmark = pytest.mark.gpu
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
per_tree = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.per_tree")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


class Pair:
    """The HIP tree and the twin driven by the same calls; every call compares what it returns and leaves behind."""

    def __init__(self, capacity, **kw):
        self.hip = per_tree.SumTree(capacity, DEV, **kw)
        self.twin = per_numpy.SumTree(capacity, **kw)
        self.C, self.pos, self.size = capacity, 0, 0

    def compare(self, what):
        tree = self.hip.tree.cpu().numpy()
        state = self.hip.state[:4].cpu().numpy()
        bad = np.flatnonzero(tree.view(np.int64) != self.twin.tree.view(np.int64))
        print(f"{what}: {len(bad)} of {len(tree)} nodes differ; state {state.tolist()} / {self.twin.state().tolist()}")
        assert len(bad) == 0, (what, bad[:8], tree[bad[:8]], self.twin.tree[bad[:8]])
        assert np.array_equal(state, self.twin.state()), what

    def add(self, n):
        self.hip.add(self.pos, n, self.size)
        self.twin.add(self.pos, n, self.size)
        self.pos, self.size = (self.pos + n) % self.C, min(self.size + n, self.C)
        self.compare(f"add {n}")

    def sample(self, u):
        idx, ring, w = self.hip.sample(torch.from_numpy(u).to(DEV), self.size)
        ti, tr, tw = self.twin.sample(u, self.size)
        idx, ring, w = idx.cpu().numpy(), ring.cpu().numpy(), w.cpu().numpy()
        assert np.array_equal(idx, ti) and np.array_equal(ring, tr), f"sample {len(u)}"
        assert ring.min() >= 0 and ring.max() < self.size and np.all(self.twin.tree[ti] > 0.0)
        ulps = np.abs(w.view(np.int32).astype(np.int64) - tw.astype(np.float32).view(np.int32).astype(np.int64))
        print(f"sample {len(u)}: weights differ by at most {ulps.max()} float32 ulp")
        assert ulps.max() <= 1
        return idx

    def update(self, idx, td):
        self.hip.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV))
        self.after_update(idx, td)

    def after_update(self, idx, td):
        """the twin's side of an update the device has done: the leaves are powers, and the device restates the C library's
        pow (csrc/per_pow.hpp), so they too are compared bitwise"""
        self.twin.update(idx, td)
        self.compare(f"update {len(idx)}")


def test_hip_replays_the_reference_trace():
    fx = np.load(os.path.join(GOLDEN, "per_trace.npz"))
    p = Pair(int(fx["capacity"]), alpha=float(fx["alpha"]), beta=float(fx["beta"]), epsilon=float(fx["epsilon"]),
             update_max_freq=int(fx["update_max_freq"]), initial_priority=float(fx["initial_priority"]))
    for step, rows in enumerate(fx["rows"]):
        p.add(int(rows))
        idx = p.sample(fx["u"][step])
        assert np.array_equal(idx, fx["indices"][step]), step        # the reference's own draw
        p.update(idx, fx["td"][step])
    stats = p.hip.stats().cpu().numpy()
    assert stats[0] == p.twin.tree[0] and stats[1] == p.twin.max_p


@pytest.mark.parametrize("capacity", [1, 3, 1000, 2 ** 20, 10 ** 6])
def test_hip_equals_the_twin_at_the_limits(capacity):
    """adds of 1, 4096 and 32 768 rows (wrapping, also more rows than the ring holds), samples of 1, 32 and 4096, updates of
    4096 rows and with all indices equal, until the ring has wrapped."""
    rng = np.random.default_rng(capacity)
    p = Pair(capacity, update_max_freq=1000)

    def round_of_samples():
        for n in (1, 32, 4096):
            idx = p.sample(rng.random(n))
            p.update(idx, (rng.standard_normal(n) * np.exp(rng.uniform(-3, 2))).astype(np.float32))
        p.update(np.full(4096, idx[0]), rng.standard_normal(4096).astype(np.float32))     # the highest row wins
        p.update(np.full(1, idx[-1]), rng.standard_normal(1).astype(np.float32))

    added = 0
    for n in (1, 4096, 32768, 1, 4096):
        p.add(n)
        added += n
        round_of_samples()
    while added <= capacity + 32768:       # big rings: fill up and wrap with the largest add
        p.add(32768)
        added += 32768
    round_of_samples()
    assert per_numpy.check_invariant(p.hip.tree.cpu().numpy())


def test_update_ignores_indices_that_are_not_leaves_and_sizes_are_checked():
    p = Pair(37)
    p.add(20)
    p.update(np.array([0, 35, 36, 72, 73, -1, 10 ** 9, 40]), np.ones(8, dtype=np.float32) * 2)
    from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError
    with pytest.raises(MpcGpuError, match="4096"):
        p.hip.sample(torch.zeros(4097, dtype=torch.float64, device=DEV), 20)
    with pytest.raises(MpcGpuError, match="n_entries"):
        p.hip.sample(torch.zeros(4, dtype=torch.float64, device=DEV), 0)
    with pytest.raises(MpcGpuError, match="pos"):
        p.hip.add(37, 1, 20)
    torch.cuda.synchronize()


def test_sample_and_update_replay_from_a_captured_graph():
    rng = np.random.default_rng(11)
    p = Pair(1000)
    p.add(600)
    p.update(np.arange(600) + 999, rng.standard_normal(600).astype(np.float32))
    u = torch.zeros(32, dtype=torch.float64, device=DEV)
    td = torch.zeros(32, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.hip.sample(u, p.size)                         # warm-up off the capture (code objects)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, ring, w = p.hip.sample(u, p.size)
        p.hip.update(idx, td)
    for _ in range(3):
        un, tdn = rng.random(32), rng.standard_normal(32).astype(np.float32)
        u.copy_(torch.from_numpy(un)); td.copy_(torch.from_numpy(tdn))
        graph.replay()
        ti, tr, tw = p.twin.sample(un, p.size)
        assert np.array_equal(idx.cpu().numpy(), ti) and np.array_equal(ring.cpu().numpy(), tr)
        p.after_update(ti, tdn)


def test_graphed_weighted_update_equals_the_eager_one():
    """The tolerance of test_graph_replayed_update_equals_the_eager_update, with a static weights input and a static TD-error
    output."""
    def batch(seed, n=64):
        g = torch.Generator().manual_seed(seed)
        return {k: v.to(DEV) for k, v in dict(obs=torch.rand(n, 46, generator=g) * 2 - 1, actions=torch.randint(0, 9, (n,), generator=g),
                                               rewards=torch.randn(n, generator=g), next_obs=torch.rand(n, 46, generator=g) * 2 - 1,
                                               dones=(torch.rand(n, generator=g) < 0.1).float(),
                                               weights=torch.rand(n, generator=g) * 0.9 + 0.1).items()}
    outs = []
    for graphed in (False, True):
        torch.manual_seed(0)
        tr = dqn_train.DqnTrainer(device=DEV, target_update_interval=3)
        if graphed:
            tr.enable_graph(64, weighted=True)
        losses, tds = [], []
        for i in range(8):
            losses.append(float((tr.update_graphed if graphed else tr.update)(batch(10 + i))))
            tds.append(tr.last_td_error.cpu().clone())
        outs.append((torch.cat([p.detach().reshape(-1) for p in tr.q_net.parameters()]).cpu(), losses, torch.stack(tds)))
    assert np.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-7)
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-7)
    assert torch.allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-6)


def ray_maps():
    fx = np.load(os.path.join(GOLDEN, "env_rays_traces.npz"))
    specs = json.loads(bytes(fx["specs_json"]).decode())
    return [rl_env.make_map(sp["boundary"], sp["static"], sp["dynamic"], sp["start"], sp["goal"], sp["path"]) for sp in specs.values()]


def flat(learner):
    return torch.cat([p.detach().reshape(-1) for p in learner.trainer.q_net.parameters()])


@pytest.mark.parametrize("use_graph", [False, True])
def test_per_learner_on_the_ray_environment_learns_and_resumes_exactly(tmp_path, use_graph):
    maps = ray_maps()

    def make(seed):
        torch.manual_seed(0)
        env = rl_env.BatchedRaysEnv([maps[i % 2] for i in range(128)], max_episode_steps=40)
        return dqn_train.DqnLearner(env, buffer_size=5000, learning_starts=1024, batch_size=32, train_freq=4,
                                    gradient_steps=4, target_update_interval=2048, seed=seed, track_episodes=False,
                                    use_graph=use_graph, per=True, per_kwargs=dict(update_max_freq=512))
    a = make(7)
    losses = []
    res = a.learn(total_timesteps=128 * 100, callback=lambda l: losses.append(l._last_loss.clone()))
    assert res["updates"] > 0 and all(math.isfinite(float(x)) for x in losses)
    assert a.buffer.size == 5000                                      # 12 800 rows through a ring of 5000
    tree = a.buffer.sum_tree.tree.cpu().numpy()
    assert per_numpy.check_invariant(tree) and np.all(tree[4999:] > 0.0)
    assert len(np.unique(tree[4999:])) > 100                          # the rows were re-prioritized
    b = make(7)
    b.learn(total_timesteps=128 * 100, stop_at=128 * 48)
    b.save(str(tmp_path / "checkpoint.pt"))
    c = make(1234)
    c.load(str(tmp_path / "checkpoint.pt"))
    c.learn(total_timesteps=128 * 100)
    assert torch.equal(flat(a), flat(c))
    assert torch.equal(a.buffer.sum_tree.tree, c.buffer.sum_tree.tree)
    assert torch.equal(a.buffer.sum_tree.state[:4], c.buffer.sum_tree.state[:4])
    assert torch.equal(a.buffer.obs, c.buffer.obs) and torch.equal(a.env.state, c.env.state)


def test_per_learner_on_the_image_environment_learns_and_resumes_exactly(tmp_path):
    maps = ray_maps()
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False

    def make(seed):
        torch.manual_seed(0)
        env = rl_env.BatchedImgsEnv([maps[i % 2] for i in range(32)], max_episode_steps=30)
        return dqn_train.DqnLearner(env, buffer_size=1000, learning_starts=256, batch_size=32, train_freq=4,
                                    gradient_steps=2, target_update_interval=512, seed=seed, track_episodes=False, per=True)
    with pytest.raises(ValueError, match="use_graph"):
        dqn_train.DqnLearner(rl_env.BatchedImgsEnv(maps[:2]), buffer_size=64, use_graph=True, per=True)
    a = make(7)
    losses = []
    res = a.learn(total_timesteps=32 * 60, callback=lambda l: losses.append(l._last_loss.clone()))
    assert res["updates"] > 0 and all(math.isfinite(float(x)) for x in losses)
    assert a.buffer.img.dtype == torch.uint8 and a.buffer.size == 1000
    assert per_numpy.check_invariant(a.buffer.sum_tree.tree.cpu().numpy())
    b = make(7)
    b.learn(total_timesteps=32 * 60, stop_at=32 * 28)
    b.save(str(tmp_path / "checkpoint.pt"))
    c = make(1234)
    c.load(str(tmp_path / "checkpoint.pt"))
    c.learn(total_timesteps=32 * 60)
    assert torch.equal(flat(a), flat(c))
    assert torch.equal(a.buffer.sum_tree.tree, c.buffer.sum_tree.tree)
    assert torch.equal(a.buffer.img, c.buffer.img)


def test_replay_buffer_with_per_kwargs_samples_updates_and_round_trips():
    """``ReplayBuffer(..., per_kwargs={})`` alone: four adds of four rows into a ring of ten."""
    dev = torch.device(DEV)
    buf = dqn_train.ReplayBuffer(10, 46, dev, per_kwargs={})
    assert dqn_train.ReplayBuffer(10, 46, dev).sum_tree is None and buf.sum_tree.capacity == 10
    for k in range(4):
        o = torch.full((4, 46), float(k), device=dev)
        buf.add(o, o + 0.5, torch.full((4,), k, device=dev), torch.full((4,), -float(k), device=dev), torch.zeros(4, device=dev))
    assert buf.size == 10 and buf.pos == 6 and per_numpy.check_invariant(buf.sum_tree.tree.cpu().numpy())
    s = buf.sample(8, torch.Generator(device=dev).manual_seed(1))
    assert list(s) == ["obs", "actions", "rewards", "next_obs", "dones", "indices", "weights"]
    # rows that are in the buffer: leaf index - (capacity - 1) is the ring position
    pos = s["indices"] - 9
    assert s["indices"].dtype == torch.int64 and int(pos.min()) >= 0 and int(pos.max()) < 10
    assert torch.equal(s["obs"], buf.obs[pos]) and torch.equal(s["next_obs"], s["obs"] + 0.5)
    assert torch.equal(s["rewards"], -s["obs"][:, 0]) and torch.equal(s["actions"].float(), s["obs"][:, 0])
    assert s["weights"].dtype == torch.float32 and s["weights"].shape == (8,)
    assert float(s["weights"].max()) == 1.0 and float(s["weights"].min()) > 0.0
    before = buf.sum_tree.tree.clone()
    buf.update_priorities(s["indices"], torch.linspace(-2.0, 2.0, 8, device=dev))
    assert not torch.equal(before, buf.sum_tree.tree) and per_numpy.check_invariant(buf.sum_tree.tree.cpu().numpy())
    sd = buf.state_dict()
    assert list(sd) == ["pos", "size", "obs", "next_obs", "actions", "rewards", "dones", "per"]
    other = dqn_train.ReplayBuffer(10, 46, dev, per_kwargs=dict(refresh_tree_freq=7))      # accepted and ignored
    other.load_state_dict(sd)
    assert torch.equal(other.sum_tree.tree, buf.sum_tree.tree) and torch.equal(other.sum_tree.state[:4], buf.sum_tree.state[:4])
    assert (other.pos, other.size) == (6, 10) and torch.equal(other.obs, buf.obs)
