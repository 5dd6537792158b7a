"""Evaluation episodes inside one launch without a GPU: the binding table of ``evaluate`` and its header, every
refusal of the entry from a process that never touches a device, the Python refusals on stand-in objects, the CPU twin of the
bookkeeping rule (tests/support/eval_numpy.py) and ``EvalCallback`` on a stand-in learner."""
import ctypes as C
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from support import eval_numpy as en
from trajtrack_mpcndqn_rlboost_amd import collect, evaluate, rl_env
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mpcgpu_[a-z_0-9]+)\s*\(", text))


# ---- binding ---------------------------------------------------------------------------------------------------------------
def test_the_built_library_and_the_header_have_exactly_these_exports():
    assert evaluate.EVAL_EXPORTS == ("mpcgpu_eval_rays_dev", "mpcgpu_eval_last_error") == tuple(evaluate._EVAL_TABLE)
    path = solver_mod.library_path()
    assert os.path.exists(path), f"{path} missing -- run __graft_entry__.build()"
    lib = C.CDLL(path)
    for sym in evaluate.EVAL_EXPORTS:
        assert hasattr(lib, sym), sym
    lib.mpcgpu_abi_version.restype = C.c_int32
    assert lib.mpcgpu_abi_version() == 8
    assert declared("mpcgpu_eval.h") == set(evaluate.EVAL_EXPORTS)
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h != "mpcgpu_eval.h"]
    assert len(others) >= 10
    for header in others:
        assert not declared(header) & set(evaluate.EVAL_EXPORTS), header
    text = open(os.path.join(ROOT, "include", "mpcgpu_eval.h")).read()
    assert int(re.search(r"#define MPCGPU_EVAL_MAX_EPISODES\s+(\d+)", text).group(1)) == evaluate.MAX_EPISODES == 256
    assert int(re.search(r"#define MPCGPU_EVAL_MAX_LAUNCH_STEPS\s+(\d+)", text).group(1)) == evaluate.MAX_LAUNCH_STEPS == 4096
    assert evaluate.DEFAULT_LAUNCH_STEPS <= evaluate.MAX_LAUNCH_STEPS
    assert C.sizeof(evaluate._CEvalParams) == 8 * 3 + 4 * 2
    # the argument counts, written out: device, params, B, 9 environment tensors, max_episode_steps, theta, eval, 4 progress
    # vectors, 3 outputs, stream
    restype, argtypes = evaluate._EVAL_TABLE["mpcgpu_eval_rays_dev"]
    assert restype is C.c_int32 and len(argtypes) == 3 + 9 + 1 + 1 + 1 + 4 + 3 + 1 == 23
    assert evaluate._EVAL_TABLE["mpcgpu_eval_last_error"] == (C.c_char_p, [])
    decl = re.search(r"int32_t mpcgpu_eval_rays_dev\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    assert len(decl.split(",")) == 23


class _Stand:
    """A library handle that lacks some exports."""
    def __init__(self, real, without):
        for name in evaluate.EVAL_EXPORTS + collect.COLLECT_EXPORTS:
            if name not in without:
                setattr(self, name, getattr(real, name))


def test_bind_refuses_a_library_without_either_export_by_name():
    real = C.CDLL(solver_mod.library_path())
    for missing in evaluate.EVAL_EXPORTS:
        with pytest.raises(MpcGpuError) as err:
            evaluate._bind(_Stand(real, {missing}))
        words = str(err.value)
        assert missing in words and "csrc/envgpu.hip" in words and "rebuild" in words and "no fallback" in words
        assert not [name for name in evaluate.EVAL_EXPORTS if name != missing and name in words]
    # a handle bound for the collect table does not stand in for eval
    half = _Stand(real, set(evaluate.EVAL_EXPORTS))
    assert collect._bind(half) is half and half._bound_tags == {"collect"}
    with pytest.raises(MpcGpuError, match="mpcgpu_eval_rays_dev"):
        evaluate._bind(half)
    whole = _Stand(real, set())
    collect._bind(whole)
    assert evaluate._bind(whole) is whole and whole._bound_tags == {"collect", "eval"}
    assert whole.mpcgpu_eval_rays_dev.restype is C.c_int32 and len(whole.mpcgpu_eval_rays_dev.argtypes) == 23


# ---- refusals of the entry: no device is touched -----------------------------------------------------------------------------
def env_params(**kw):
    base = dict(n_path_max=4, n_obst_max=2, n_kf_max=2, n_edge_max=16, num_segments=8, corner_samples=3, time_step=0.2,
                sample_offset=0.0, collision_factor=4.0, reach_goal_factor=3.0, cross_track_factor=0.05,
                excessive_speed_factor=4.0, reference_speed=1.2, path_progress_factor=2.0, **rl_env.ROBOT)
    base.update(kw)
    return rl_env._CParams(**base)


def eval_params(E=2, S=8, eps=0.0):
    return evaluate._CEvalParams(eps=eps, seed=1, serial0=0, episodes=E, max_steps=S)


def test_refusals_of_the_entry_need_no_device_and_leave_the_arrays():
    """Every refusal comes before the device is touched (this process has none), with the entry's own error text; the seven
    arrays, here host memory with a pattern, keep every byte."""
    lib = evaluate._bind(solver_mod.load_library())
    B, E = 8, 2
    p = 4096                                                       # any non-null address: a refused call reads none of them
    env_ptrs = ["records", "state", "obs_internal", "obs_external", "reward", "terminated", "truncated", "term_internal", "term_external"]
    rng = np.random.default_rng(1)
    arrays = {name: rng.integers(1, 100, B).astype(dtype) for name, dtype in en.PROGRESS}
    arrays.update({name: rng.integers(1, 100, (B, E)).astype(dtype) for name, dtype in en.OUTPUTS})
    before = {k: v.copy() for k, v in arrays.items()}
    seven = [name for name, _ in en.PROGRESS + en.OUTPUTS]
    assert len(seven) == 7

    def rays(params=None, B=B, max_steps=3, ep=None, **null):
        a = {k: (None if k in null else p) for k in env_ptrs + ["theta"]}
        a.update({k: (None if k in null else arrays[k].ctypes.data) for k in seven})
        params = env_params() if params is None else params
        ep = eval_params() if ep is None else ep
        return lib.mpcgpu_eval_rays_dev(0, C.byref(params) if params != "null" else None, B, *(a[k] for k in env_ptrs), max_steps,
                                        a["theta"], C.byref(ep) if ep != "null" else None, *(a[k] for k in seven), None)
    nan = float("nan")
    cases = [(dict(**{k: True}), "null pointer (an environment tensor)") for k in env_ptrs]
    cases += [(dict(theta=True), "null pointer (theta / eval)"), (dict(ep="null"), "null pointer (theta / eval)")]
    cases += [(dict(**{k: True}), "null pointer (episodes_done / steps_done / ep_return / ep_length)") for k in seven[:4]]
    cases += [(dict(**{k: True}), "null pointer (returns / lengths / outcome)") for k in seven[4:]]
    cases += [(dict(params="null"), "invalid mpcgpu_env_params"), (dict(B=-1), "negative batch"),
              (dict(ep=eval_params(E=0)), "1 <= episodes <= 256"), (dict(ep=eval_params(E=257)), "1 <= episodes <= 256"),
              (dict(ep=eval_params(E=-3)), "1 <= episodes <= 256"),
              (dict(ep=eval_params(S=0)), "1 <= max_steps <= 4096"), (dict(ep=eval_params(S=4097)), "1 <= max_steps <= 4096"),
              (dict(ep=eval_params(eps=-0.1)), "eps must lie in [0, 1]"), (dict(ep=eval_params(eps=1.1)), "eps must lie in [0, 1]"),
              (dict(ep=eval_params(eps=nan)), "eps must lie in [0, 1]"),
              (dict(max_steps=0), "max_episode_steps must be positive"), (dict(max_steps=-5), "max_episode_steps must be positive"),
              (dict(params=env_params(n_path_max=65)), "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
              (dict(params=env_params(n_obst_max=32)), "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
              (dict(params=env_params(num_segments=16)), "only num_segments = 8 and corner_samples = 3 are built"),
              (dict(params=env_params(corner_samples=2)), "only num_segments = 8 and corner_samples = 3 are built")]
    for kw, text in cases:
        assert rays(**kw) < 0 and text in lib.mpcgpu_eval_last_error().decode(), (kw, lib.mpcgpu_eval_last_error())
        assert all(np.array_equal(arrays[k], before[k]) for k in arrays), kw
    # the ends of the ranges are inside, and an empty batch is nothing to do
    for ep in (eval_params(E=1, S=1), eval_params(E=256, S=4096, eps=1.0)):
        assert rays(B=0, ep=ep) == 0
    # the words of the environment's own entry for the same params, each in its own slot
    env_lib = rl_env._bind(lib)
    bad = env_params(num_segments=16)
    assert env_lib.mpcgpu_env_step_autoreset_dev(0, C.byref(bad), 8, p, p, p, p, p, p, p, p, p, p, 3, None) < 0
    assert rays(params=bad) < 0 and lib.mpcgpu_eval_last_error() == env_lib.mpcgpu_env_last_error()
    collect_lib = collect._bind(lib)
    said = collect_lib.mpcgpu_collect_last_error()
    assert rays(B=-1) < 0 and collect_lib.mpcgpu_collect_last_error() == said
    assert all(np.array_equal(arrays[k], before[k]) for k in arrays)


# ---- refusals in Python, on stand-in objects ------------------------------------------------------------------------------
def _stub_env(**kw):
    base = dict(B=4, device=torch.device("cpu"), is_image_env=False, records2=None, max_episode_steps=3)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_python_refusals_on_stand_in_objects():
    theta = torch.zeros(1177)
    with pytest.raises(ValueError, match="ray environment only.*image environment is out of its scope"):
        evaluate.evaluate_rays(_stub_env(is_image_env=True), theta, 1)
    with pytest.raises(ValueError, match="enable_spares.*two-record table is out of its scope"):
        evaluate.evaluate_rays(_stub_env(records2=torch.zeros(2, 4, 4)), theta, 1)
    for n in (0, -1):
        with pytest.raises(ValueError, match="n_episodes must be at least 1"):
            evaluate.evaluate_rays(_stub_env(), theta, n)
    with pytest.raises(ValueError, match="launch_steps must be at least 1"):
        evaluate.evaluate_rays(_stub_env(), theta, 1, launch_steps=0)
    for wrong in (theta[:100], theta.double(), theta.reshape(11, 107), torch.zeros(2 * 1177)[::2], "theta"):
        with pytest.raises(ValueError, match="theta must be at least 1177 contiguous float32"):
            evaluate.evaluate_rays(_stub_env(), wrong, 1)
    with pytest.raises(ValueError, match=r"progress\['steps_done'\]"):
        evaluate.evaluate_rays(_stub_env(), theta, 1, progress=dict(evaluate.new_progress(4, "cpu"), steps_done=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"out\['returns'\] must be 4 x 2"):
        evaluate.evaluate_rays(_stub_env(), theta, 2, out={"returns": torch.zeros(4, 3, dtype=torch.float64)})
    # the callback checks its environment and its numbers when it is made
    with pytest.raises(ValueError, match="ray environment only"):
        evaluate.EvalCallback(_stub_env(is_image_env=True), 100)
    with pytest.raises(ValueError, match="enable_spares"):
        evaluate.EvalCallback(_stub_env(records2=torch.zeros(2, 4, 4)), 100)
    with pytest.raises(ValueError, match="eval_freq"):
        evaluate.EvalCallback(_stub_env(), 0)
    with pytest.raises(ValueError, match="n_eval_episodes"):
        evaluate.EvalCallback(_stub_env(), 100, n_eval_episodes=257)
    assert evaluate.launches_that_suffice(1, 400, 1024) == 1 and evaluate.launches_that_suffice(3, 400, 1024) == 2
    assert evaluate.launches_that_suffice(256, 1000, 1) == 256000 and evaluate.launches_that_suffice(2, 3, 4) == 2


# ---- the twin of the bookkeeping rule --------------------------------------------------------------------------------------
def scripts(B, steps, limit=5, seed=0):
    """Row b: rewards of its own, episodes that end after ``1 + (b + i) % limit`` steps, alternately terminated (flags 1, 2, 4 in
    turn) and truncated (flags 0); row 0 only truncates, every ``limit`` steps."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        row, length, i = [], 0, 0
        for s in range(steps):
            length += 1
            want = limit if b == 0 else 1 + (b + i) % limit
            if length == want:
                truncated = b == 0 or i % 2 == 1
                row.append((float(rng.normal()), not truncated, truncated, 0 if truncated else (1, 2, 4)[(b + i) % 3] | 16))
                length, i = 0, i + 1
            else:
                row.append((float(rng.normal()), False, False, 0))
        out.append(row)
    return out


def run(script, E, launches, fill=77):
    progress, out, serials = en.new_progress(len(script)), en.new_out(len(script), E, fill), [[] for _ in script]
    trips = [en.launch(script, progress, out, E, S, serial0=1000, serials=serials) for S in launches]
    return progress, out, serials, trips


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_twin_parks_rows_and_leaves_unfinished_slots():
    B, E, limit = 7, 3, 5
    script = scripts(B, E * limit)
    progress, out, serials, trips = run(script, E, [E * limit])
    assert (progress["episodes_done"] == E).all() and not progress["ep_length"].any() and not progress["ep_return"].any()
    assert trips == [int(progress["steps_done"].sum())] and np.array_equal(progress["steps_done"], out["lengths"].sum(axis=1))
    assert progress["steps_done"][0] == E * limit and len(set(progress["steps_done"].tolist())) > 2    # rows park at different trips
    assert (out["outcome"][0] == 8).all() and set(out["outcome"].reshape(-1).tolist()) == {1, 2, 4, 8}  # & 7: bit 4 of the flags is gone
    for b in range(B):                                          # the returns are the sums of the script's rewards, in order
        at = 0
        for e in range(E):
            acc = np.float64(0.0)
            for r, *_ in script[b][at:at + out["lengths"][b, e]]:
                acc = np.float64(acc + r)
            assert out["returns"][b, e] == acc
            at += out["lengths"][b, e]
    # a launch on an all-parked progress reads and writes nothing: not even a script that is gone
    kept_p, kept_o = {k: v.copy() for k, v in progress.items()}, {k: v.copy() for k, v in out.items()}
    assert en.launch([None] * B, progress, out, E, 100) == 0 and same(progress, kept_p) and same(out, kept_o)
    # cut short: slots e >= episodes_done keep the pattern, the others are written
    progress, out, _, _ = run(script, E, [4], fill=77)
    done = progress["episodes_done"]
    assert 0 < done.sum() < B * E and (done < E).any()
    for b in range(B):
        for name, _ in en.OUTPUTS:
            assert (out[name][b, done[b]:] == 77).all(), (b, name)
        assert (out["lengths"][b, :done[b]] != 77).all()
    assert progress["ep_length"][0] == 4 and progress["ep_return"][0] != 0.0 and done[0] == 0


def test_twin_split_launches_equal_one_and_the_serial_is_serial0_plus_steps_done():
    B, E, limit = 7, 3, 5
    script = scripts(B, E * limit)
    whole = run(script, E, [E * limit])
    for launches in ([1] * (E * limit), [2, E * limit - 2], [7, 8], [4096], [4, 4, 4, 4]):
        assert sum(launches) >= E * limit
        split = run(script, E, launches)
        assert same(split[0], whole[0]) and same(split[1], whole[1]) and split[2] == whole[2], launches
        assert sum(split[3]) == sum(whole[3])
    for b, row in enumerate(whole[2]):
        assert row == [1000 + i for i in range(int(whole[0]["steps_done"][b]))]
    # the stream wraps modulo 2^64 like the kernel's unsigned sum
    progress, out, serials = en.new_progress(1), en.new_out(1, 1), [[]]
    en.launch(scripts(1, 5), progress, out, 1, 5, serial0=2 ** 64 - 2, serials=serials)
    assert serials[0] == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1, 2]


def test_twin_reaches_the_bound_on_a_row_that_only_truncates():
    for E, limit, S in ((3, 5, 4), (1, 400, 1024), (2, 3, 4), (4, 3, 1), (5, 7, 35)):
        script = scripts(2, E * limit, limit=limit)
        bound = en.launches_that_suffice(E, limit, S)
        assert bound == evaluate.launches_that_suffice(E, limit, S) == -(-E * limit // S)
        progress, out = en.new_progress(2), en.new_out(2, E)
        made = 0
        while not (progress["episodes_done"] >= E).all():
            en.launch(script, progress, out, E, S)
            made += 1
        assert made == bound and progress["steps_done"][0] == E * limit      # row 0 needs every one of them


# ---- EvalCallback on a stand-in learner and a stand-in evaluate_rays ---------------------------------------------------------
class _Learner:
    def __init__(self):
        self.num_timesteps, self.saved = 0, []
        self.trainer = types.SimpleNamespace(theta=lambda: torch.full((1177,), float(self.num_timesteps)))

    def save_model(self, path):
        self.saved.append((path, self.num_timesteps))
        torch.save({"at": self.num_timesteps}, path)


def _stand_in(monkeypatch, means, B=4, E=2):
    calls = []
    env = _stub_env(B=B, resets=0)
    env.reset = lambda: setattr(env, "resets", env.resets + 1)

    def fake(e, theta, n_episodes, eps=0.0, seed=0, serial=0, launch_steps=None, **kw):
        assert e is env and n_episodes == E and not kw
        k = len(calls)
        calls.append(dict(theta=float(theta[0]), eps=eps, seed=seed, serial=serial, launch_steps=launch_steps, resets=env.resets))
        returns = means[k] + torch.arange(B * E, dtype=torch.float64).reshape(B, E) - (B * E - 1) / 2
        outcome = torch.tensor([4, 8] * (B * E // 2), dtype=torch.uint8).reshape(B, E)
        return dict(returns=returns, lengths=torch.full((B, E), 3 + k, dtype=torch.int32), outcome=outcome, success=(outcome & 4) != 0,
                    progress=None)
    monkeypatch.setattr(evaluate, "evaluate_rays", fake)
    return env, calls


def test_callback_fires_once_per_crossed_multiple_and_writes_the_reference_log(monkeypatch, tmp_path):
    means = [1.0, 3.0, 2.0, 3.0, 5.0]
    env, calls = _stand_in(monkeypatch, means)
    cb = evaluate.EvalCallback(env, eval_freq=100, n_eval_episodes=2, eps=0.0, best_model_save_path=str(tmp_path / "best"),
                               log_path=str(tmp_path / "log"), launch_steps=64, seed=9)
    assert (cb.n_evaluations, cb.last_mean_reward, cb.best_mean_reward) == (0, -float("inf"), -float("inf"))
    lr = _Learner()
    fired = []
    # rounds of 32 steps; then one jump over two multiples (300 and 400), then a call exactly on a multiple, then one past it
    for now in [32, 64, 96, 128, 160, 192, 224, 256, 288, 420, 452, 500, 532, 600]:
        lr.num_timesteps = now
        before = cb.n_evaluations
        cb(lr)
        if cb.n_evaluations != before:
            fired.append(now)
    assert fired == [128, 224, 420, 500, 600] and cb.n_evaluations == 5      # 420 crossed 300 and 400: one evaluation
    assert [c["theta"] for c in calls] == [128.0, 224.0, 420.0, 500.0, 600.0]        # the weights of that moment
    assert [c["resets"] for c in calls] == [1, 2, 3, 4, 5]                       # reset first, every time
    assert all(c["seed"] == 9 and c["eps"] == 0.0 and c["launch_steps"] == 64 for c in calls)
    assert [c["serial"] for c in calls] == [0, 6, 12, 18, 24]                    # a stream of its own, moved on by E * max_episode_steps
    assert cb.last_mean_reward == 5.0 and cb.best_mean_reward == 5.0
    # best_model.pt on improvement only: 1, 3, (2: no), (3: no, not greater), 5
    best = str(tmp_path / "best" / "best_model.pt")
    assert lr.saved == [(best, 128), (best, 224), (best, 600)] and torch.load(best)["at"] == 600
    # the file: the reference's keys and dtypes, plus successes
    z = np.load(str(tmp_path / "log" / "evaluations.npz"))
    assert set(z.files) == {"timesteps", "results", "ep_lengths", "successes"}
    assert z["timesteps"].dtype == np.int64 and z["timesteps"].shape == (5,) and z["timesteps"].tolist() == fired
    assert z["results"].dtype == np.float64 and z["results"].shape == (5, 8)
    assert z["ep_lengths"].dtype == np.int64 and z["ep_lengths"].shape == (5, 8) and z["ep_lengths"][:, 0].tolist() == [3, 4, 5, 6, 7]
    assert z["successes"].dtype == np.bool_ and z["successes"].shape == (5, 8) and z["successes"][0].tolist() == [True, False] * 4
    assert np.allclose(z["results"].mean(axis=1), means) and z["results"][0].tolist() == [1.0 + i - 3.5 for i in range(8)]   # row-major over [B, E]


def test_callback_without_paths_writes_nothing_and_a_state_dict_continues_the_log(monkeypatch, tmp_path):
    means = [1.0, 3.0, 2.0, 4.0]
    env, calls = _stand_in(monkeypatch, means)
    lr = _Learner()
    quiet = evaluate.EvalCallback(env, 100, n_eval_episodes=2)
    lr.num_timesteps = 100
    quiet(lr)
    assert quiet.n_evaluations == 1 and lr.saved == [] and not os.listdir(tmp_path)
    calls.clear()
    env.resets = 0
    first = evaluate.EvalCallback(env, 100, n_eval_episodes=2, log_path=str(tmp_path), best_model_save_path=str(tmp_path), seed=5)
    for now in (96, 128, 224):
        lr.num_timesteps = now
        first(lr)
    d = first.state_dict()

    def plain(v):
        return isinstance(v, (int, float, bool, torch.Tensor)) or (isinstance(v, list) and all(plain(x) for x in v))
    assert all(plain(v) for v in d.values())
    torch.save(d, str(tmp_path / "cb.pt"))
    second = evaluate.EvalCallback(env, 100, n_eval_episodes=2, log_path=str(tmp_path), best_model_save_path=str(tmp_path), seed=77)
    second.load_state_dict(torch.load(str(tmp_path / "cb.pt"), weights_only=True))
    assert (second.seed, second.serial, second.n_evaluations, second.best_mean_reward) == (5, 12, 2, 3.0)
    lr.saved.clear()
    for now in (256, 288, 320, 410):        # 256, 288: no new multiple since 224; 320 and 410 cross one each
        lr.num_timesteps = now
        second(lr)
    assert second.n_evaluations == 4 and [c["serial"] for c in calls] == [0, 6, 12, 18] and all(c["seed"] == 5 for c in calls)
    z = np.load(str(tmp_path / "evaluations.npz"))
    assert z["timesteps"].tolist() == [128, 224, 320, 410] and np.allclose(z["results"].mean(axis=1), means)
    assert [at for _, at in lr.saved] == [410]                   # 2.0 is no improvement on the restored best of 3.0; 4.0 is


def test_training_tool_takes_eval_freq():
    sys.path.insert(0, ROOT)
    train_dqn = importlib.import_module("tools.train_dqn")
    off = train_dqn.parse_args([])
    assert off.eval_freq == 0
    on = train_dqn.parse_args(["--fused", "--collect-in-kernel", "--eval-freq", "5000", "--eval-envs", "32", "--eval-episodes", "2"])
    assert (on.eval_freq, on.eval_envs, on.eval_episodes) == (5000, 32, 2)
    with pytest.raises(SystemExit) as err:
        train_dqn.parse_args(["--eval-freq", "100", "--images"])
    assert err.value.code == 2
