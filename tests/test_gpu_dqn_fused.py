"""The fused DQN update on the GPU (csrc/dqngpu.hip): every entry of include/mpcgpu_dqn.h bit for bit against
the numpy twin (tests/support/dqn_numpy.py), the equalities between the entries, the refusals, and the paths of
``FusedDqnTrainer`` / ``DqnLearner(fused=True)`` against the parent's trainer, RCCL, a checkpoint and a captured graph."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from support import dqn_cases, dqn_numpy as tw
from trajtrack_mpcndqn_rlboost_amd import dqn_fused, dqn_train, rl_env
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NP, F = tw.NP, np.float32
EDGE = dqn_cases.edge_cases()


def make(theta, target, double_q=False, **kw):
    tr = dqn_fused.FusedDqnTrainer(device=DEV, double_q=double_q, target_update_interval=0, **kw)
    with torch.no_grad():
        tr.state[:NP] = torch.from_numpy(theta).to(DEV)
        tr.state[NP:2 * NP] = torch.from_numpy(target).to(DEV)
    return tr


def make_set(theta, target, kw, **more):
    """A trainer at a set of tests/support/dqn_cases.py PARAMETER_SETS: lr, gamma, max_grad_norm and double_q are keywords of
    ``FusedDqnTrainer``; beta1, beta2 and eps are fields of its ``params`` (what every entry passes to the library)."""
    tr = make(theta, target, **{k: v for k, v in kw.items() if k in ("lr", "gamma", "max_grad_norm", "double_q")}, **more)
    for k in ("beta1", "beta2", "eps"):
        if k in kw:
            setattr(tr.params, k, kw[k])
    return tr


def on_device(batch):
    return {k: torch.from_numpy(v).to(DEV) for k, v in batch.items()}


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, F)
    return np.ascontiguousarray(x, F).reshape(-1).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_state_is(tr, twin):
    s = tr.state.cpu().numpy()
    assert same(s[:NP], twin.theta) and same(s[NP:2 * NP], twin.target), "parameters"
    assert same(s[2 * NP:3 * NP], twin.m) and same(s[3 * NP:4 * NP], twin.v), "moments"
    assert tr.step_count == twin.t


def walk(theta, target, batches, double_q=False, t0=None, kw=None):
    """Every batch through (a) grad_dev then apply_dev, (b) step_dev and (c) the twin: gradient, loss, delta after the gradient,
    parameters, moments and step count after the step, all bit for bit; (a) and (b) also against each other.  ``kw``: a set of
    dqn_cases.PARAMETER_SETS (the defaults otherwise)."""
    kw = dict(kw or {}, double_q=(kw or {}).get("double_q", double_q))
    two, one, twin = make_set(theta, target, kw), make_set(theta, target, kw), tw.Twin(theta, target, **kw)
    if t0 is not None:          # a checkpoint: moments and a step count in the form of Adam's state_dict
        rng = np.random.default_rng(1)
        twin.m, twin.v, twin.t = (0.1 * rng.standard_normal(NP)).astype(F), (rng.random(NP) ** 4).astype(F), t0
        groups = dqn_fused.adam_groups(two.params.lr)
        groups[0].update(betas=(two.params.beta1, two.params.beta2), eps=two.params.eps)
        sd = dqn_fused.adam_state_dict(torch.from_numpy(twin.m), torch.from_numpy(twin.v), t0, groups)
        two.load_optimizer_state(sd); one.load_optimizer_state(sd)
        assert_state_is(two, twin)
    for batch in batches:
        n = len(batch["actions"])
        g, loss, d = twin.grad(batch["obs"], batch["next_obs"], batch["actions"], batch["rewards"], batch["dones"], batch.get("weights"))
        before = two.state.clone()
        grad = two.grad(on_device(batch))
        assert same(grad, g) and same(two._loss, loss) and same(two.last_td_error, d) and two.last_td_error.numel() == n
        assert torch.equal(two.state, before)                         # grad_dev leaves the state alone
        two.apply(grad)
        twin.apply(g)
        assert_state_is(two, twin)
        assert same(one.update(on_device(batch)), loss) and same(one._bucket, g) and same(one.last_td_error, d)
        assert torch.equal(one.state, two.state)                      # step_dev == grad_dev + apply_dev
    return twin


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("n", dqn_cases.SIZES)
def test_entries_equal_the_twin(n, weights):
    rng = np.random.default_rng(1000 + n)
    twin = walk(dqn_cases.random_theta(rng), dqn_cases.random_theta(rng),
                [dqn_cases.random_batch(rng, n, weights=weights) for _ in range(2)], double_q=n % 2 == 1)
    assert twin.t == 2


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_batches_equal_the_twin(name):
    c = EDGE[name]
    twin = walk(c["theta"], c["target"], [c["batch"], c["batch"]], c["double_q"])
    if name == "dead_hidden":           # zero gradients below the dead layer: the Adam step there is 0 / (0 + eps)
        assert same(twin.theta[:tw.OFF_W2], c["theta"][:tw.OFF_W2]) and not twin.m[:tw.OFF_W2].any()


@pytest.mark.parametrize("t0", [0, 10 ** 6])
def test_step_counts_one_and_a_million(t0):
    rng = np.random.default_rng(77)
    twin = walk(dqn_cases.random_theta(rng), dqn_cases.random_theta(rng), [dqn_cases.random_batch(rng, 32)], t0=t0 or None)
    assert twin.t == t0 + 1


@pytest.mark.parametrize("name", sorted(dqn_cases.PARAMETER_SETS))
def test_every_parameter_set_equals_the_twin(name):
    """Two batches of 33 rows, the second with weights, at every set of the table: from t = 0 and, where a beta moved, from
    checkpoints at t = 999 and t = 10^6 (there beta^t leaves the restated pow's range: 0.5^999 and every beta^(10^6) but
    0.9999^(10^6) go through the device library's pow, the latter to an underflow)."""
    kw = dqn_cases.PARAMETER_SETS[name]
    for t0 in (None, 999, 10 ** 6) if dqn_cases.moves_a_beta(kw) else (None,):
        rng = np.random.default_rng(300)
        batches = [dqn_cases.random_batch(rng, 33), dqn_cases.random_batch(rng, 33, weights=True)]
        twin = walk(dqn_cases.random_theta(rng), dqn_cases.random_theta(rng), batches, t0=t0, kw=kw)
        assert twin.t == (t0 or 0) + 2
        print(f"{name}, t0 = {t0 or 0}: gradient, loss, delta, theta, m, v and t equal the twin's bit for bit (0 differing bits)")


def test_all_moved_train_equals_single_steps_and_the_twin():
    """``train`` with K = 3, n = 32 on 33 rows at the set that moves everything: against single steps and the twin's loop."""
    kw = dqn_cases.PARAMETER_SETS["all_moved"]
    K, n, size = 3, 32, 33
    rng = np.random.default_rng(K + size + n)
    theta, target = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng)
    buf, host = make_buffer(rng, size, capacity=size + 7)
    seed, serial0 = 2 ** 63 + 11, 2 ** 40 + 5
    fused, steps = make_set(theta, target, kw, seed=seed), make_set(theta, target, kw)
    fused.serial = serial0
    losses = fused.train(buf, K, n)
    assert fused.serial == serial0 + K and fused.num_updates == K and losses.shape == (K,)
    want = []
    for s in range(K):
        rows = torch.from_numpy(tw.sample_rows(seed, serial0 + s, n, size)).to(DEV)
        want.append(steps.update(buf._rows(rows)).clone())
    assert torch.equal(fused.state, steps.state) and fused.step_count == K
    assert same(losses, torch.stack(want))
    twin = tw.Twin(theta, target, **kw)
    assert same(losses, twin.train(host, size, n, K, seed, serial0))
    assert_state_is(fused, twin)


def test_invalid_parameters_are_refused_and_leave_the_state_alone():
    """Every rule of mpcgpu_dqn_params through the C ABI, on all four entries: the text names the structure and its rules, and
    neither the state block nor an output is written."""
    rng = np.random.default_rng(5)
    theta = dqn_cases.random_theta(rng)
    tr = make(theta, theta)
    buf, _ = make_buffer(rng, 64)
    b = on_device(dqn_cases.random_batch(rng, 8))
    tr.update(b)                                                             # a state with moments in it
    before, outs = tr.state.clone(), (tr._bucket.clone(), tr._loss.clone(), tr._td.clone())
    lib, losses, st = tr._lib, torch.zeros(4, device=DEV), torch.cuda.current_stream().cuda_stream
    good = dict(lr=1e-4, gamma=0.98, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8, double_q=0)
    bad = [dict(lr=0.0), dict(lr=-1e-4), dict(lr=float("nan")), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(eps=0.0),
           dict(eps=-1e-8), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=float("nan")),
           dict(double_q=2), dict(double_q=-1)]
    for change in bad:
        f = dict(good, **change)
        p = dqn_fused._CDqnParams(f["lr"], f["gamma"], f["max_grad_norm"], f["beta1"], f["beta2"], f["eps"], f["double_q"], 0)
        mini = (b["obs"].data_ptr(), b["next_obs"].data_ptr(), b["actions"].data_ptr(), b["rewards"].data_ptr(), b["dones"].data_ptr(), None,
                8, tr._bucket.data_ptr(), tr._loss.data_ptr(), tr._td.data_ptr(), st)
        calls = (lambda: lib.mpcgpu_dqn_grad_dev(0, C.byref(p), tr.state.data_ptr(), *mini),
                 lambda: lib.mpcgpu_dqn_step_dev(0, C.byref(p), tr.state.data_ptr(), *mini),
                 lambda: lib.mpcgpu_dqn_apply_dev(0, C.byref(p), tr.state.data_ptr(), tr._bucket.data_ptr(), 1.0, st),
                 lambda: lib.mpcgpu_dqn_train_dev(0, C.byref(p), tr.state.data_ptr(), buf.obs.data_ptr(), buf.next_obs.data_ptr(),
                                                  buf.actions.data_ptr(), buf.rewards.data_ptr(), buf.dones.data_ptr(), 64, 8, 2, 1, 0,
                                                  losses.data_ptr(), st))
        for call in calls:
            lib.mpcgpu_dqn_grad_dev(0, C.byref(tr.params), tr.state.data_ptr(), *mini[:6], 0, *mini[7:])    # another text in between
            assert "1 <= n <= 256" in lib.mpcgpu_dqn_last_error().decode()
            assert call() < 0, change
            text = lib.mpcgpu_dqn_last_error().decode()
            assert "invalid mpcgpu_dqn_params" in text and "lr, max_grad_norm, eps > 0" in text and "0 <= beta < 1" in text \
                and "double_q 0 / 1" in text, (change, text)
    torch.cuda.synchronize()
    assert torch.equal(tr.state, before) and all(torch.equal(x, y) for x, y in zip((tr._bucket, tr._loss, tr._td), outs))
    assert not losses.any() and tr.step_count == 1


def test_scaled_apply_equals_the_twin():
    rng = np.random.default_rng(8)
    theta = dqn_cases.random_theta(rng)
    tr, twin = make(theta, theta), tw.Twin(theta)
    for scale in (0.5, 1.0 / 3.0, 1.0 / 8.0):
        g = rng.standard_normal(NP).astype(F)
        tr.apply(torch.from_numpy(g).to(DEV), scale)
        twin.apply(g, scale)
        assert_state_is(tr, twin)


# ---- K steps in one launch ---------------------------------------------------------------------------------------------------
def make_buffer(rng, size, capacity=None):
    buf = dqn_train.ReplayBuffer(capacity or size, 46, torch.device(DEV))
    b = dqn_cases.random_batch(rng, size)
    buf.add(*(torch.from_numpy(b[k]).to(DEV) for k in ("obs", "next_obs", "actions", "rewards", "dones")))
    return buf, b


@pytest.mark.parametrize("n", [32, 256])
@pytest.mark.parametrize("size", [1, 33, 1000])
@pytest.mark.parametrize("K", [1, 2, 50])
def test_train_equals_single_steps_on_the_sampled_rows(K, size, n):
    rng = np.random.default_rng(K + size + n)
    theta, target = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng)
    buf, host = make_buffer(rng, size, capacity=size + 7)
    seed, serial0 = 2 ** 63 + 11, 2 ** 40 + 5
    fused, steps = make(theta, target, seed=seed), make(theta, target)
    fused.serial = serial0
    losses = fused.train(buf, K, n)
    assert fused.serial == serial0 + K and fused.num_updates == K and losses.shape == (K,)
    want = []
    for s in range(K):
        rows = torch.from_numpy(tw.sample_rows(seed, serial0 + s, n, size)).to(DEV)
        want.append(steps.update(buf._rows(rows)).clone())
    assert torch.equal(fused.state, steps.state) and fused.step_count == K
    assert same(losses, torch.stack(want))
    if K == 2:                                                       # ... and the twin's own K-step loop
        twin = tw.Twin(theta, target)
        assert same(losses, twin.train(host, size, n, K, seed, serial0))
        assert_state_is(fused, twin)


def test_two_train_launches_equal_one():
    rng = np.random.default_rng(4)
    theta, target = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng)
    buf, _ = make_buffer(rng, 1000)
    whole, halves = make(theta, target, seed=9), make(theta, target, seed=9)
    a = whole.train(buf, 50, 32)
    b = torch.cat([halves.train(buf, 25, 32), halves.train(buf, 25, 32)])
    assert torch.equal(whole.state, halves.state) and same(a, b) and whole.serial == halves.serial == 50


def test_refusals_enqueue_nothing():
    rng = np.random.default_rng(6)
    theta = dqn_cases.random_theta(rng)
    tr = make(theta, theta)
    buf, _ = make_buffer(rng, 64)
    tr.update(on_device(dqn_cases.random_batch(rng, 8)))                     # a state with moments in it
    before, outs = tr.state.clone(), (tr._bucket.clone(), tr._loss.clone())
    for n in (0, 257):
        for entry in (tr.update, tr.grad):
            with pytest.raises(MpcGpuError, match="1 <= n <= 256"):
                entry(on_device(dqn_cases.random_batch(rng, n)))
    lib, losses = tr._lib, torch.zeros(4, device=DEV)

    def train(size, n, K, state=tr.state.data_ptr()):
        return lib.mpcgpu_dqn_train_dev(0, C.byref(tr.params), state, buf.obs.data_ptr(), buf.next_obs.data_ptr(), buf.actions.data_ptr(),
                                        buf.rewards.data_ptr(), buf.dones.data_ptr(), size, n, K, 1, 0, losses.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    for args, text in (((64, 32, 0), "1 <= K <= 65536"), ((64, 32, 65537), "1 <= K <= 65536"), ((0, 32, 1), "1 <= size < 2^31"),
                       ((2 ** 31, 32, 1), "1 <= size < 2^31"), ((64, 0, 1), "1 <= n <= 256"), ((64, 257, 1), "1 <= n <= 256")):
        assert train(*args) < 0 and text in lib.mpcgpu_dqn_last_error().decode(), args
    assert train(64, 32, 1, state=None) < 0 and "null pointer" in lib.mpcgpu_dqn_last_error().decode()
    assert lib.mpcgpu_dqn_apply_dev(0, C.byref(tr.params), tr.state.data_ptr(), None, 1.0, None) < 0
    buf.size = 0
    with pytest.raises(MpcGpuError, match="1 <= size"):
        tr.train(buf, 1, 32)
    torch.cuda.synchronize()
    assert torch.equal(tr.state, before) and torch.equal(tr._bucket, outs[0]) and torch.equal(tr._loss, outs[1])
    assert not losses.any() and tr.num_updates == 1 and tr.serial == 0


# ---- against the parent's trainer ------------------------------------------------------------------------------------------------
def test_gradient_is_as_close_to_float64_as_the_eager_trainer():
    rng = np.random.default_rng(21)
    theta, target, batch = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng), dqn_cases.random_batch(rng, 32)
    exact = dqn_cases.torch_gradient(theta, target, batch, dtype=torch.float64)
    eager = dqn_cases.torch_gradient(theta, target, batch, device=DEV)       # DqnTrainer's own float32 backward on the GPU
    fused = make(theta, target).grad(on_device(batch)).cpu().numpy().astype(np.float64)
    E, mine = np.abs(eager - exact).max(), np.abs(fused - exact).max()
    print(f"eager DqnTrainer off by E = {E:.3e}, fused gradient by {mine:.3e} (ratio {mine / E:.2f})")
    assert mine <= 4.0 * E


def test_adam_state_moves_between_the_trainers_both_ways():
    rng = np.random.default_rng(22)
    theta, target = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng)
    batches = [dqn_cases.random_batch(rng, 32) for _ in range(3)]
    eager = dqn_cases.torch_trainer(theta, target, device=DEV)
    for b in batches[:2]:
        eager.update(dqn_cases.torch_batch(b, device=DEV))
    fused = make(theta, target)
    fused.q_net.load_state_dict(eager.q_net.state_dict())
    fused.load_optimizer_state(eager.optimizer.state_dict())                   # DqnTrainer -> FusedDqnTrainer
    assert fused.step_count == 2
    assert torch.equal(fused.state[:NP], torch.cat([p.detach().reshape(-1) for p in eager.q_net.parameters()]))
    sd = fused.optimizer.state_dict()
    for i, p in enumerate(eager.q_net.parameters()):
        assert torch.equal(sd["state"][i]["exp_avg"], eager.optimizer.state[p]["exp_avg"].cpu())
        assert torch.equal(sd["state"][i]["exp_avg_sq"], eager.optimizer.state[p]["exp_avg_sq"].cpu())
    fused.update(on_device(batches[2]))
    eager.update(dqn_cases.torch_batch(batches[2], device=DEV))
    flat = torch.cat([p.detach().reshape(-1) for p in eager.q_net.parameters()])
    assert torch.allclose(fused.state[:NP], flat, rtol=1e-5, atol=1e-7)       # the same step, each in its own float32 order
    back = dqn_cases.torch_trainer(theta, target, device=DEV)                  # FusedDqnTrainer -> DqnTrainer
    back.q_net.load_state_dict(fused.q_net.state_dict())
    back.load_optimizer_state(fused.optimizer.state_dict())
    assert float(back.optimizer.state[next(back.q_net.parameters())]["step"]) == 3
    back.update(dqn_cases.torch_batch(batches[0], device=DEV))
    fused.update(on_device(batches[0]))
    assert torch.allclose(fused.state[:NP], torch.cat([p.detach().reshape(-1) for p in back.q_net.parameters()]), rtol=1e-5, atol=1e-7)
    # the views are the block: greedy actions of q_net follow the kernel's parameters
    obs = torch.from_numpy(batches[0]["obs"]).to(DEV)
    assert torch.equal(fused.q_net.greedy_actions(obs), back.q_net.greedy_actions(obs))
    fused.sync_target()
    assert torch.equal(fused.state[NP:2 * NP], fused.state[:NP]) and fused.q_net_target.q_net[0].weight.data_ptr() == fused.state[NP:].data_ptr()


def test_collective_path_equals_the_single_launch():
    """gradient kernel -> RCCL all-reduce -> apply kernel (one-rank process group, force_collective) == step kernel, bitwise."""
    script = os.path.join(ROOT, "tests", "support", "rccl_one_rank_fused.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "== fused step over 6 updates, bit for bit" in r.stdout


def test_captured_train_call_replays_to_the_same_bits():
    rng = np.random.default_rng(23)
    theta, target = dqn_cases.random_theta(rng), dqn_cases.random_theta(rng)
    buf, _ = make_buffer(rng, 500)
    eager, graphed = make(theta, target, seed=3), make(theta, target, seed=3)
    want = eager.train(buf, 8, 32)
    graphed.grad(buf._rows(torch.arange(4, device=DEV)))             # the kernel is loaded before the capture; the state is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = graphed.train(buf, 8, 32)
    torch.cuda.synchronize()
    assert graphed.step_count == 0                                   # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.state, eager.state) and same(got, want) and graphed.step_count == 8


# ---- the learner -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "env_rays_traces.npz"))
    specs = json.loads(bytes(fx["specs_json"]).decode())
    return [rl_env.make_map(sp["boundary"], sp["static"], sp["dynamic"], sp["start"], sp["goal"], sp["path"]) for sp in specs.values()]


def test_fused_learner_follows_the_sb3_counters(maps):
    torch.manual_seed(0)
    env = rl_env.BatchedRaysEnv([maps[i % 2] for i in range(64)], max_episode_steps=40)
    learner = dqn_train.DqnLearner(env, buffer_size=8192, learning_starts=512, batch_size=32, train_freq=4, gradient_steps=-1,
                                   target_update_interval=1024, seed=5, fused=True)
    assert isinstance(learner.trainer, dqn_fused.FusedDqnTrainer) and learner.trainer.seed == 5
    w0 = learner.trainer.state[:NP].clone()
    stats = learner.learn(total_timesteps=64 * 60)
    tr = learner.trainer
    assert stats["timesteps"] == 3840 and learner.n_calls == 60 and learner.buffer.size == 3840
    # gradient_steps = -1: one update per collected transition once learning has started; each round of 256 was ONE launch
    assert stats["updates"] == 3840 - 512 == tr.num_updates == tr.step_count == tr.serial
    assert tr.num_target_syncs == 60 // (1024 // 64)                 # hard target sync every 1024 environment steps
    assert np.isfinite(stats["loss"]) and stats["episodes"] >= 64 and not torch.equal(w0, tr.state[:NP])
    assert torch.isfinite(tr.state).all()


@pytest.mark.parametrize("per", [False, True])
def test_resumed_fused_run_equals_the_uninterrupted_run(maps, per):
    def make_learner(seed):
        torch.manual_seed(0)
        env = rl_env.BatchedRaysEnv([maps[i % 2] for i in range(64)], max_episode_steps=40)
        return dqn_train.DqnLearner(env, buffer_size=8192, learning_starts=512, batch_size=32, train_freq=4,
                                    gradient_steps=8 if per else -1, target_update_interval=1024, seed=seed, track_episodes=False,
                                    per=per, fused=True)
    a = make_learner(7)
    a.learn(total_timesteps=64 * 60)
    b = make_learner(7)
    b.learn(total_timesteps=64 * 60, stop_at=64 * 28)
    file = io.BytesIO()
    torch.save(b.state_dict(), file)
    file.seek(0)
    c = make_learner(1234)
    c.load_state_dict(torch.load(file, map_location=DEV, weights_only=True))
    assert c.trainer.seed == 7 and c.trainer.serial == b.trainer.serial
    c.learn(total_timesteps=64 * 60)
    assert torch.equal(a.trainer.state, c.trainer.state) and a.trainer.step_count > 0       # parameters, target, moments, t
    assert a.trainer.serial == c.trainer.serial and a.trainer.num_updates == c.trainer.num_updates
    n = a.buffer.size
    assert c.buffer.size == n and c.buffer.pos == a.buffer.pos
    for k in ("obs", "next_obs", "actions", "rewards", "dones"):
        assert torch.equal(getattr(a.buffer, k)[:n], getattr(c.buffer, k)[:n]), k
    if per:
        assert torch.equal(a.buffer.sum_tree.tree, c.buffer.sum_tree.tree)
    assert torch.equal(a.env.state, c.env.state) and float(a.ep_count) == float(c.ep_count) > 0
