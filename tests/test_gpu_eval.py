"""Evaluation episodes inside one launch on the GPU (include/mpcgpu_eval.h).

The defining property -- for every row the launch leaves the state, the environment's outputs, the progress vectors and the three
[B, E] outputs that driving the row from the host leaves (``collect.act`` -> ``env.step(auto_reset=True)`` -> the bookkeeping
of the header), every bit of them, with each row's tensors taken at the round its E-th episode ended --; split launches, a
launch on parked rows, ``sync=False``, graph replay, the seed, untouched slots, refusals, the two trainers' parameter vectors,
and ``EvalCallback`` in ``DqnLearner.learn``.

Environments: tests/support/collect_cases.py after a reset (``max_episode_steps = 3``; row b is of kind b mod 3: an episode of
exactly 3 steps that ends at the time limit, of 1 step, of up to 3 steps that ends at the goal or in a wall).  So every row has
its E episodes within 3 E steps and rows park at different trips; both are asserted from the outputs, with the census of
outcomes."""
import numpy as np
import pytest
import torch

from support import collect_cases as cc, dqn_cases, eval_numpy as en
from trajtrack_mpcndqn_rlboost_amd import collect, dqn_fused, dqn_train, evaluate, rl_env
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV_TENSORS = ("state", "obs_internal", "obs_external", "reward", "terminated", "truncated", "term_internal", "term_external")
PROGRESS = tuple(name for name, _ in evaluate.PROGRESS)
OUT_NAMES = tuple(name for name, _ in evaluate.OUTPUTS)
SEED = 0x5EED_0000_0000_0002
SERIAL = 2 ** 40 + 5
LIMIT = cc.MAX_EPISODE_STEPS


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not same_bits(a[k], b[k])]


def theta_of(seed=3) -> torch.Tensor:
    return torch.from_numpy(dqn_cases.random_theta(np.random.default_rng(seed))).to(DEV)


def make_env(B):
    env = rl_env.BatchedRaysEnv(cc.maps(B), max_episode_steps=LIMIT)
    env.reset()
    return env


def new_out(B, E, fill=0):
    """The three [B, E] outputs, every slot holding a pattern no episode leaves (``fill`` = 0: zeros)."""
    return {name: torch.full((B, E), fill, dtype=dtype, device=DEV) for name, dtype in evaluate.OUTPUTS}


def snapshot(env, progress, out):
    d = {"env." + k: getattr(env, k).clone() for k in ENV_TENSORS}
    d.update({"progress." + k: progress[k].clone() for k in PROGRESS})
    d.update({"out." + k: out[k].clone() for k in OUT_NAMES})
    return d


def restore(snap, env, progress, out):
    for k in ENV_TENSORS:
        getattr(env, k).copy_(snap["env." + k])
    for k in PROGRESS:
        progress[k].copy_(snap["progress." + k])
    for k in OUT_NAMES:
        out[k].copy_(snap["out." + k])


def host_driven(B, E, eps, theta, fill=0):
    """3 E rounds of the public single-step pieces on all rows (rows do not see each other, so a row driven with the others is
    the row driven alone), the header's bookkeeping in torch operations on the rows that still play, and each row's environment
    tensors taken at the round its E-th episode ended -> a snapshot in the form of :func:`snapshot`."""
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E, fill)
    final = {k: torch.zeros_like(getattr(env, k)) for k in ENV_TENSORS}
    live = torch.ones(B, dtype=torch.bool, device=DEV)
    rows = torch.arange(B, device=DEV)
    for r in range(LIMIT * E):
        # every live row has made r steps: its serial SERIAL + steps_done is SERIAL + r
        assert bool((progress["steps_done"][live] == r).all())
        actions = collect.act(env, theta, eps, SEED, SERIAL + r)
        env.step(actions, auto_reset=True)
        flags = env.state[:, 26].to(torch.int64)
        truncated, ended = env.truncated.bool(), (env.terminated.bool() | env.truncated.bool()) & live
        progress["ep_return"].copy_(torch.where(live, progress["ep_return"] + env.reward, progress["ep_return"]))
        progress["ep_length"] += live.to(torch.int32)
        progress["steps_done"] += live.to(torch.int64)
        at, slot = rows[ended], progress["episodes_done"][ended].long()
        out["returns"][at, slot] = progress["ep_return"][ended]
        out["lengths"][at, slot] = progress["ep_length"][ended]
        out["outcome"][at, slot] = ((flags & 7) | (truncated.to(torch.int64) * 8)).to(torch.uint8)[ended]
        progress["ep_return"][ended] = 0.0
        progress["ep_length"][ended] = 0
        progress["episodes_done"] += ended.to(torch.int32)
        parked = live & (progress["episodes_done"] >= E)
        for k in ENV_TENSORS:
            final[k][parked] = getattr(env, k)[parked]
        live = live & ~parked
    assert not bool(live.any())                       # every row has its E episodes within 3 E steps
    d = {"env." + k: final[k] for k in ENV_TENSORS}
    d.update({"progress." + k: progress[k] for k in PROGRESS})
    d.update({"out." + k: out[k] for k in OUT_NAMES})
    return d


def launched(B, E, eps, theta, steps=None, fill=0, seed=SEED, serial=SERIAL):
    """The same evaluation as launches of ``steps`` (default: one launch of 3 E) -> a snapshot."""
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E, fill)
    for S in (steps or [LIMIT * E]):
        evaluate.launch_rays(env, theta, E, S, progress, out, eps=eps, seed=seed, serial=serial)
    return snapshot(env, progress, out)


def assert_census(snap, B, E):
    """From the outputs: the row kinds, rows that park at different trips, terminations and truncations."""
    lengths, outcome = snap["out.lengths"].cpu().numpy(), snap["out.outcome"].cpu().numpy()
    steps, kinds = snap["progress.steps_done"].cpu().numpy(), np.arange(B) % 3
    assert (snap["progress.episodes_done"].cpu().numpy() == E).all()
    assert not snap["progress.ep_length"].any() and not snap["progress.ep_return"].any()
    assert np.array_equal(steps, lengths.sum(axis=1)) and steps.max() <= LIMIT * E
    assert (lengths[kinds == 0] == LIMIT).all() and (outcome[kinds == 0] == 8).all()                 # the time limit, nothing else
    assert (lengths[kinds == 1] == 1).all() and ((outcome[kinds == 1] & 7) != 0).all() and ((outcome[kinds == 1] & 8) == 0).all()
    assert ((lengths[kinds == 2] >= 1) & (lengths[kinds == 2] <= LIMIT)).all()    # (a row whose goal lies at a wall can end at once)
    assert (((outcome & 7) != 0) != ((outcome & 8) != 0)).all()               # an episode ends one way or the other
    terminations, truncations = int(((outcome & 7) != 0).sum()), int(((outcome & 8) != 0).sum())
    print(f"B {B} E {E}: terminations {terminations}, truncations {truncations}, goals {int(((outcome & 4) != 0).sum())}, "
          f"steps per row {steps.min()} .. {steps.max()}")
    if B >= 5:
        assert terminations >= 1 and truncations >= 1
        assert steps[0] == LIMIT * E and steps[1] == E and len(set(steps.tolist())) >= 2          # rows park at different trips
    else:
        assert truncations == E and terminations == 0        # the one row is a time-limit row


# ---- the defining property ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.37])
@pytest.mark.parametrize("E", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 5, 64, 257])
def test_a_launch_equals_every_row_driven_from_the_host(B, E, eps):
    theta = theta_of()
    host = host_driven(B, E, eps, theta, fill=0)
    launch = launched(B, E, eps, theta, fill=0)
    assert differing(launch, host) == []
    assert_census(host, B, E)
    if eps > 0.0 and B >= 64:           # the evaluation held explored and greedy steps
        steps = host["progress.steps_done"].tolist()
        explored = [en.explored(SEED, SERIAL, range(steps[b]), b, eps) for b in range(B)]
        assert any(explored) and not all(explored)


# ---- launches ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole():
    """One launch of 3 E steps at B = 64, E = 2, eps = 0.37: what the other ways of launching must give."""
    return launched(64, 2, 0.37, theta_of())


def test_split_launches_equal_one_launch(whole):
    B, E, theta = 64, 2, theta_of()
    for steps in ([1] * (LIMIT * E), [2, LIMIT * E - 2], [4096]):
        assert differing(launched(B, E, 0.37, theta, steps=steps), whole) == [], steps
    assert_census(whole, B, E)


def test_a_launch_on_parked_rows_changes_nothing(whole):
    B, E, theta = 64, 2, theta_of()
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E)
    restore(whole, env, progress, out)
    # another theta, eps, seed and serial: a parked row reads none of them
    evaluate.launch_rays(env, theta_of(8), E, 4096, progress, out, eps=1.0, seed=1, serial=2)
    res = evaluate.evaluate_rays(env, theta_of(8), E, eps=1.0, progress=progress, out=out)
    torch.cuda.synchronize()
    assert differing(snapshot(env, progress, out), whole) == []
    assert res["progress"] is progress and res["returns"] is out["returns"]


def test_sync_false_equals_sync_true(whole):
    B, E, theta = 64, 2, theta_of()
    for launch_steps, launches in ((None, 1), (4, 2), (1, 6), (10 ** 6, 1)):
        assert evaluate.launches_that_suffice(E, LIMIT, min(launch_steps or 1024, 4096)) == launches
        for sync in (True, False):
            env = make_env(B)
            res = evaluate.evaluate_rays(env, theta, E, eps=0.37, seed=SEED, serial=SERIAL, launch_steps=launch_steps, sync=sync)
            assert differing(snapshot(env, res["progress"], res), whole) == [], (launch_steps, sync)
            assert torch.equal(res["success"], (res["outcome"] & 4) != 0) and res["success"].dtype == torch.bool


def test_a_captured_evaluation_replays_to_the_same_bits(whole):
    B, E, theta = 64, 2, theta_of()
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E)
    start = snapshot(env, progress, out)
    evaluate.evaluate_rays(env, theta, E, eps=0.37, seed=SEED, serial=SERIAL, launch_steps=4, progress=progress, out=out, sync=False)
    assert differing(snapshot(env, progress, out), whole) == []
    restore(start, env, progress, out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        evaluate.evaluate_rays(env, theta, E, eps=0.37, seed=SEED, serial=SERIAL, launch_steps=4, progress=progress, out=out, sync=False)
    restore(start, env, progress, out)
    graph.replay()
    torch.cuda.synchronize()
    assert differing(snapshot(env, progress, out), whole) == []


def test_the_seed_moves_explored_rows_only():
    B, E, theta = 64, 1, theta_of()        # one episode: rows of 1 to 3 steps, a dozen of which explore under neither seed
    a, b = launched(B, E, 0.0, theta, seed=1), launched(B, E, 0.0, theta, seed=2)
    assert differing(a, b) == []                                          # eps = 0 never draws
    eps, seeds = 0.37, (SEED, SEED + 1)
    a, b = (launched(B, E, eps, theta, seed=s) for s in seeds)
    steps = a["progress.steps_done"].tolist()
    # a row that explores under neither seed in the steps it made plays the same steps under both (by induction over its steps)
    explored = np.array([any(en.explored(s, SERIAL, range(steps[r]), r, eps) for s in seeds) for r in range(B)])
    assert 5 <= explored.sum() <= B - 5
    moved = np.zeros(B, bool)
    for k in a:
        x, y = (v[k].reshape(B, -1).contiguous().view(torch.uint8).reshape(B, -1) for v in (a, b))
        moved |= (x != y).any(dim=1).cpu().numpy()
    assert not (moved & ~explored).any() and moved.any()


def test_slots_of_unfinished_episodes_keep_what_they_held():
    B, E, theta, fill = 64, 4, theta_of(), 113
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E, fill)
    evaluate.launch_rays(env, theta, E, 2, progress, out, eps=0.37, seed=SEED, serial=SERIAL)      # cut short: two steps per row
    done = progress["episodes_done"].cpu().numpy()
    kinds = np.arange(B) % 3
    assert (done[kinds == 0] == 0).all() and (done[kinds == 1] == 2).all() and set(done[kinds == 2].tolist()) <= {0, 1, 2}
    assert (done < E).all() and len(set(done.tolist())) >= 2
    assert (progress["steps_done"] == 2).all()
    for name in OUT_NAMES:
        x = out[name].cpu().numpy()
        for b in range(B):
            assert (x[b, done[b]:] == fill).all(), (name, b)
    assert (out["lengths"].cpu().numpy()[kinds == 1, :2] == 1).all()
    # the rest of the evaluation from there equals the evaluation in one launch
    evaluate.evaluate_rays(env, theta, E, eps=0.37, seed=SEED, serial=SERIAL, progress=progress, out=out)
    assert differing(snapshot(env, progress, out), launched(B, E, 0.37, theta, fill=fill)) == []


def test_refusals_leave_everything_as_it_was():
    B, E, theta = 5, 2, theta_of()
    env, progress, out = make_env(B), evaluate.new_progress(B, DEV), new_out(B, E, 113)
    progress["steps_done"] += 7
    before = snapshot(env, progress, out)
    nan = float("nan")
    for kw, text in ((dict(steps=0), None), (dict(steps=4097), r"1 <= max_steps <= 4096"), (dict(eps=1.5), r"eps must lie in \[0, 1\]"),
                     (dict(eps=-0.1), r"eps must lie in \[0, 1\]"), (dict(eps=nan), r"eps must lie in \[0, 1\]")):
        with pytest.raises(ValueError if text is None else MpcGpuError, match=text or "launch_steps"):
            evaluate.launch_rays(env, theta, E, kw.get("steps", 3), progress, out, eps=kw.get("eps", 0.0), seed=SEED)
    with pytest.raises(MpcGpuError, match="1 <= episodes <= 256"):
        evaluate.evaluate_rays(env, theta, 257, progress=progress)
    env.max_episode_steps = 0
    with pytest.raises(MpcGpuError, match="max_episode_steps must be positive"):
        evaluate.launch_rays(env, theta, E, 3, progress, out)
    env.max_episode_steps = LIMIT
    with pytest.raises(ValueError, match="theta"):
        evaluate.evaluate_rays(env, theta[:100], E, progress=progress, out=out)
    with pytest.raises(ValueError, match=r"out\['lengths'\]"):
        evaluate.evaluate_rays(env, theta, E, progress=progress, out=dict(out, lengths=out["lengths"].long()))
    torch.cuda.synchronize()
    assert differing(snapshot(env, progress, out), before) == []
    spares = make_env(3)
    spares.enable_spares()
    with pytest.raises(ValueError, match="enable_spares"):
        evaluate.evaluate_rays(spares, theta, 1)


def test_both_trainers_hand_over_the_same_parameters():
    B, E = 64, 2
    torch.manual_seed(5)
    fused = dqn_fused.FusedDqnTrainer(device=DEV, seed=4)
    plain = dqn_train.DqnTrainer(device=DEV)
    plain.q_net.load_state_dict(fused.q_net.state_dict())
    assert fused.theta() is fused.state and fused.state.numel() > 1177                  # the state block begins with theta
    assert same_bits(plain.theta(), fused.state[:1177].clone()) and plain.theta().numel() == 1177
    sides = []
    for theta in (plain.theta(), fused.theta()):
        env = make_env(B)
        res = evaluate.evaluate_rays(env, theta, E)
        sides.append(snapshot(env, res["progress"], res))
    assert differing(*sides) == []
    assert_census(sides[0], B, E)


# ---- the learner -----------------------------------------------------------------------------------------------------------
def learner(**kw):
    torch.manual_seed(1)
    env = rl_env.BatchedRaysEnv(cc.maps(8), max_episode_steps=LIMIT)
    return dqn_train.DqnLearner(env, buffer_size=512, learning_starts=24, batch_size=16, train_freq=4, gradient_steps=2,
                                target_update_interval=40, seed=4, **kw)


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
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) or same_bits(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


@pytest.mark.parametrize("setting", [dict(fused=False), dict(fused=True, collect_in_kernel=True)], ids=["host_driven", "fused_collect_in_kernel"])
def test_a_run_with_the_callback_is_the_run_without(setting, tmp_path):
    B_eval, E, total = 6, 2, 320
    without, with_cb = learner(**setting), learner(**setting)
    without.learn(total)
    maps = cc.maps(B_eval, seed=1)
    eval_env = rl_env.BatchedRaysEnv(maps, max_episode_steps=LIMIT)
    cb = evaluate.EvalCallback(eval_env, eval_freq=100, n_eval_episodes=E, best_model_save_path=str(tmp_path), log_path=str(tmp_path), seed=11)
    moments, evaluate_now = [], cb.evaluate

    def recording(lr):           # what the evaluation starts from: the environment's state, the weights, the serial
        moments.append((eval_env.state_dict(), lr.trainer.theta()[:1177].clone(), cb.serial))
        return evaluate_now(lr)
    cb.evaluate = recording
    stats = with_cb.learn(total, callback=cb)
    assert stats["timesteps"] == total and stats["updates"] > 0
    assert_same_checkpoint(with_cb.state_dict(), without.state_dict())
    assert same_bits(with_cb.trainer.theta()[:1177].clone(), without.trainer.theta()[:1177].clone())
    assert with_cb.buffer.size == without.buffer.size == total
    # rounds of 4 x 8 steps end at 32, 64, ...: the multiples of 100 are passed at 128, 224 and 320
    assert cb.n_evaluations == 3 and cb.timesteps == [128, 224, 320] and [m[2] for m in moments] == [0, E * LIMIT, 2 * E * LIMIT]
    z = np.load(str(tmp_path / "evaluations.npz"))
    assert z["timesteps"].tolist() == [128, 224, 320] and z["results"].shape == (3, B_eval * E) and z["ep_lengths"].shape == (3, B_eval * E)
    assert z["results"].dtype == np.float64 and z["ep_lengths"].dtype == np.int64 and z["successes"].dtype == np.bool_
    assert cb.best_mean_reward == z["results"].mean(axis=1).max() and cb.last_mean_reward == z["results"][-1].mean()
    assert (tmp_path / "best_model.pt").exists()
    # every logged row is a direct evaluation on a reset copy of the evaluation environment with the weights of that moment
    assert not torch.equal(moments[0][1], moments[-1][1])
    for k, (state, theta, serial) in enumerate(moments):
        copy = rl_env.BatchedRaysEnv(maps, max_episode_steps=LIMIT)
        copy.load_state_dict(state)
        copy.reset()
        res = evaluate.evaluate_rays(copy, theta, E, seed=11, serial=serial)
        assert np.array_equal(res["returns"].reshape(-1).cpu().numpy(), z["results"][k]), k
        assert np.array_equal(res["lengths"].reshape(-1).cpu().numpy(), z["ep_lengths"][k]), k
        assert np.array_equal(res["success"].reshape(-1).cpu().numpy(), z["successes"][k]), k
    kinds = np.arange(B_eval * E) // E % 3
    assert (z["ep_lengths"][:, kinds == 0] == LIMIT).all() and (z["ep_lengths"][:, kinds == 1] == 1).all()
