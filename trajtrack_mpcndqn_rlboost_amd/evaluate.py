"""Evaluation episodes inside one launch: host side of ``include/mpcgpu_eval.h``.

:func:`evaluate_rays` lets every row of a :class:`rl_env.BatchedRaysEnv` play ``n_episodes`` episodes to their end with the
policy of ``include/mpcgpu_collect.h`` -- greedy with ``eps = 0``, SB3's ``model.predict(deterministic=True)`` -- in launches
of ``csrc/envgpu.hip`` that make up to ``launch_steps`` steps per row: bit for bit what :func:`collect.act`,
``env.step(auto_reset=True)`` and the episode bookkeeping do per row when they are driven from the host, without the launches
around every step.  :class:`EvalCallback` is what the reference's training run builds on SB3's class of that name
(src/test_block_rl.py:65-99): periodic evaluation on a separate environment, ``best_model.pt`` by the mean evaluation return
and ``evaluations.npz``.  There is no fallback in torch operations: without the kernel the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from .collect import _theta
from .rl_env import _CParams
from .solver import MpcGpuError, bind_exports

MAX_EPISODES = 256
MAX_LAUNCH_STEPS = 4096
DEFAULT_LAUNCH_STEPS = 1024
PROGRESS = (("episodes_done", torch.int32), ("steps_done", torch.int64), ("ep_return", torch.float64), ("ep_length", torch.int32))
OUTPUTS = (("returns", torch.float64), ("lengths", torch.int32), ("outcome", torch.uint8))
# bits of ``outcome``
OBSTACLE_COLLISION, BOUNDARY_COLLISION, GOAL_REACHED, TIME_LIMIT = 1, 2, 4, 8


class _CEvalParams(C.Structure):
    _fields_ = [("eps", C.c_double), ("seed", C.c_uint64), ("serial0", C.c_uint64), ("episodes", C.c_int32), ("max_steps", C.c_int32)]


_VP, _I32 = C.c_void_p, C.c_int32
# export -> (restype, argtypes); include/mpcgpu_eval.h
_EVAL_TABLE = {
    "mpcgpu_eval_rays_dev": (_I32, [_I32, C.POINTER(_CParams), _I32] + [_VP] * 9 + [_I32, _VP, C.POINTER(_CEvalParams)] + [_VP] * 8),
    "mpcgpu_eval_last_error": (C.c_char_p, []),
}
EVAL_EXPORTS = tuple(_EVAL_TABLE)


def _bind(lib):
    return bind_exports(lib, "eval", _EVAL_TABLE, "csrc/envgpu.hip")


def check_env(env) -> None:
    """What the kernel is built for: the ray environment on one record table.  Raises ``ValueError`` otherwise."""
    if getattr(env, "is_image_env", False):
        raise ValueError("evaluation inside the launch is built for the ray environment only: the image environment is out of "
                         "its scope (its observation is drawn by a second kernel)")
    if getattr(env, "records2", None) is not None:
        raise ValueError("evaluation inside the launch is not built for an environment after enable_spares() / "
                         "enable_fresh_maps(): the two-record table is out of its scope")


def launches_that_suffice(n_episodes: int, max_episode_steps: int, launch_steps: int) -> int:
    """``ceil(E * max_episode_steps / S)``: no row needs more steps than E episodes of full length."""
    return -(-int(n_episodes) * int(max_episode_steps) // int(launch_steps))


def new_progress(B: int, device) -> Dict[str, torch.Tensor]:
    """The progress vectors of an evaluation that begins: all zero."""
    return {name: torch.zeros(B, dtype=dtype, device=device) for name, dtype in PROGRESS}


def _checked(group: str, given: Optional[Dict[str, torch.Tensor]], spec, shape, device) -> Dict[str, torch.Tensor]:
    for name, dtype in spec:
        x = None if given is None else given.get(name)
        if (not isinstance(x, torch.Tensor) or x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous()
                or x.device != device):
            raise ValueError(f"{group}[{name!r}] must be {' x '.join(map(str, shape))} contiguous {dtype} values on {device}")
    return given


def _launcher(env, theta: torch.Tensor, E: int, S: int, eps: float, seed: int, serial: int, progress, out):
    """The checks of one evaluation -> a function that enqueues ONE launch of S steps per row and raises on a refusal."""
    check_env(env)
    B, device = env.B, env.device
    if E < 1:
        raise ValueError(f"n_episodes must be at least 1, got {E}")
    if S < 1:
        raise ValueError(f"launch_steps must be at least 1, got {S}")
    theta = _theta(theta, device)
    _checked("progress", progress, PROGRESS, (B,), device)
    _checked("out", out, OUTPUTS, (B, E), device)
    p = _CEvalParams(eps=float(eps), seed=int(seed) % 2 ** 64, serial0=int(serial) % 2 ** 64, episodes=E,
                     max_steps=S if S <= MAX_LAUNCH_STEPS else MAX_LAUNCH_STEPS + 1)
    lib = _bind(env._lib)
    args = (env.device_index, C.byref(env.params), B, env.records.data_ptr(), env.state.data_ptr(), env.obs_internal.data_ptr(),
            env.obs_external.data_ptr(), env.reward.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
            env.term_internal.data_ptr(), env.term_external.data_ptr(), int(env.max_episode_steps), theta.data_ptr(), C.byref(p),
            *(progress[name].data_ptr() for name, _ in PROGRESS), *(out[name].data_ptr() for name, _ in OUTPUTS))

    def launch() -> None:
        if lib.mpcgpu_eval_rays_dev(*args, torch.cuda.current_stream(device).cuda_stream) != 0:
            raise MpcGpuError(lib.mpcgpu_eval_last_error().decode())
    return launch


def launch_rays(env, theta: torch.Tensor, n_episodes: int, steps: int, progress: Dict[str, torch.Tensor],
                out: Dict[str, torch.Tensor], eps: float = 0.0, seed: int = 0, serial: int = 0) -> None:
    """ONE launch of ``mpcgpu_eval_rays_dev``: every row that has fewer than ``n_episodes`` episodes in ``progress`` makes up to
    ``steps`` (1 .. 4096) steps; ``progress`` (:func:`new_progress`) and ``out`` (``returns``, ``lengths``, ``outcome``, each
    [B, E]) are updated in place.  Nothing is read back."""
    _launcher(env, theta, int(n_episodes), int(steps), eps, seed, serial, progress, out)()


def evaluate_rays(env, theta: torch.Tensor, n_episodes: int, eps: float = 0.0, seed: int = 0, serial: int = 0,
                  launch_steps: Optional[int] = None, progress: Optional[Dict[str, torch.Tensor]] = None,
                  out: Optional[Dict[str, torch.Tensor]] = None, sync: bool = True) -> Dict[str, torch.Tensor]:
    """Every row of ``env`` plays ``n_episodes`` (1 .. 256) episodes to their end, acting by the rule of
    ``include/mpcgpu_collect.h`` with ``eps`` on the counter stream ``(seed, serial + the row's own step count)``.

    The environment is NOT reset: the rows play from where ``env`` stands, and the caller decides (``env.reset()`` first for
    an evaluation from the start states).  ``progress=None`` begins an evaluation with zeroed progress vectors; the returned
    ``progress`` continues one (for instance after :func:`launch_rays`).  ``launch_steps`` (default 1024, capped at 4096) is
    what a row steps in one launch.  With ``sync=True`` launches follow each other until every row has its episodes, with one
    host read per launch; with ``sync=False`` ``ceil(n_episodes * max_episode_steps / launch_steps)`` launches are enqueued and
    nothing is read -- that number always suffices, a row that is finished costs its wavefront an early return, and the call
    can be captured into a graph.

    Returns ``returns`` [B, E] float64, ``lengths`` [B, E] int32, ``outcome`` [B, E] uint8 (bit 0 obstacle collision, bit 1
    boundary collision, bit 2 goal reached, bit 3 time limit), ``success`` [B, E] bool (bit 2 of ``outcome``) and ``progress``.
    ``out`` may bring the three [B, E] tensors; slots of episodes a row has not finished keep what they held.  Refusals come
    before anything is enqueued and leave every tensor as it was."""
    check_env(env)
    E = int(n_episodes)
    S = DEFAULT_LAUNCH_STEPS if launch_steps is None else min(int(launch_steps), MAX_LAUNCH_STEPS)
    if E >= 1 and progress is None:
        progress = new_progress(env.B, env.device)
    if E >= 1 and out is None:
        out = {name: torch.zeros(env.B, E, dtype=dtype, device=env.device) for name, dtype in OUTPUTS}
    launch = _launcher(env, theta, E, S, eps, seed, serial, progress, out)
    for _ in range(launches_that_suffice(E, max(int(env.max_episode_steps), 1), S)):
        launch()
        if sync and bool((progress["episodes_done"] >= E).all()):
            break
    result = {name: out[name] for name, _ in OUTPUTS}
    result["success"] = (out["outcome"] & GOAL_REACHED) != 0
    result["progress"] = progress
    return result


class EvalCallback:
    """Periodic evaluation for ``DqnLearner.learn(callback=...)``: what the reference's run does with SB3's ``EvalCallback``.

    Whenever ``learner.num_timesteps`` has passed a multiple of ``eval_freq`` since the last call, ONE evaluation runs (one,
    also when a round jumped over several multiples): ``eval_env.reset()``, ``theta = learner.trainer.theta()``,
    :func:`evaluate_rays` with ``n_eval_episodes`` per row.  Its ``B * E`` returns, lengths and successes (row-major over
    ``[B, E]``) are appended to the log together with ``num_timesteps``; when the mean return exceeds the best so far and
    ``best_model_save_path`` is given, ``learner.save_model(<path>/best_model.pt)``; when ``log_path`` is given,
    ``<log_path>/evaluations.npz`` is rewritten with the keys and dtypes of the reference's files -- ``timesteps`` int64 [n],
    ``results`` float64 [n, B * E], ``ep_lengths`` int64 [n, B * E] -- and ``successes`` bool [n, B * E], which SB3 adds when
    the info has ``is_success``.

    ``eval_freq`` counts ENVIRONMENT STEPS (``num_timesteps``).  SB3's ``eval_freq`` counts calls of the vectorised
    environment, ``n_envs`` steps each: SB3's ``eval_freq = f`` on ``n`` environments is ``eval_freq = f * n`` here.

    The callback draws from ``(seed, serial)`` of its own (``serial`` moves on by ``n_eval_episodes * max_episode_steps`` per
    evaluation, more than any row steps) and reads nothing but ``num_timesteps`` and the weights: it never touches the
    learner's generator, ``collect_serial`` or ``fused_serial``, so a run with the callback is the same run as without.  Its
    state is its own (``state_dict`` / ``load_state_dict``: tensors, numbers and lists), not part of the learner's checkpoint.

    Several ranks: each rank evaluates its own environment with its own callback, and nothing is reduced across ranks."""

    def __init__(self, eval_env, eval_freq: int, n_eval_episodes: int = 1, eps: float = 0.0,
                 best_model_save_path: Optional[str] = None, log_path: Optional[str] = None,
                 launch_steps: Optional[int] = None, seed: int = 0):
        if int(eval_freq) < 1:
            raise ValueError(f"eval_freq must be at least 1 environment step, got {eval_freq}")
        if not 1 <= int(n_eval_episodes) <= MAX_EPISODES:
            raise ValueError(f"n_eval_episodes must lie in 1 .. {MAX_EPISODES}, got {n_eval_episodes}")
        check_env(eval_env)
        self.eval_env, self.eval_freq, self.n_eval_episodes, self.eps = eval_env, int(eval_freq), int(n_eval_episodes), float(eps)
        self.best_model_save_path, self.log_path, self.launch_steps = best_model_save_path, log_path, launch_steps
        self.seed, self.serial = int(seed) % 2 ** 64, 0
        self.last_eval_timestep = 0
        self.last_mean_reward, self.best_mean_reward = -float("inf"), -float("inf")
        self.timesteps, self.results, self.ep_lengths, self.successes = [], [], [], []

    @property
    def n_evaluations(self) -> int:
        return len(self.timesteps)

    def __call__(self, learner) -> None:
        now = int(learner.num_timesteps)
        if now // self.eval_freq > self.last_eval_timestep // self.eval_freq:
            self.last_eval_timestep = now
            self.evaluate(learner)

    def evaluate(self, learner) -> Dict[str, torch.Tensor]:
        """One evaluation now, logged at ``learner.num_timesteps``."""
        env = self.eval_env
        env.reset()
        res = evaluate_rays(env, learner.trainer.theta(), self.n_eval_episodes, eps=self.eps, seed=self.seed, serial=self.serial,
                            launch_steps=self.launch_steps)
        self.serial += self.n_eval_episodes * int(env.max_episode_steps)
        self.timesteps.append(int(learner.num_timesteps))
        self.results.append(res["returns"].reshape(-1).cpu().tolist())
        self.ep_lengths.append(res["lengths"].reshape(-1).cpu().tolist())
        self.successes.append(res["success"].reshape(-1).cpu().tolist())
        self.last_mean_reward = float(np.mean(self.results[-1]))
        if self.last_mean_reward > self.best_mean_reward:
            self.best_mean_reward = self.last_mean_reward
            if self.best_model_save_path is not None:
                os.makedirs(self.best_model_save_path, exist_ok=True)
                learner.save_model(os.path.join(self.best_model_save_path, "best_model.pt"))
        if self.log_path is not None:
            os.makedirs(self.log_path, exist_ok=True)
            np.savez(os.path.join(self.log_path, "evaluations.npz"), **self.log())
        return res

    def log(self) -> Dict[str, np.ndarray]:
        """The arrays of ``evaluations.npz``."""
        n = len(self.timesteps)
        return dict(timesteps=np.asarray(self.timesteps, np.int64).reshape(n),
                    results=np.asarray(self.results, np.float64).reshape(n, -1),
                    ep_lengths=np.asarray(self.ep_lengths, np.int64).reshape(n, -1),
                    successes=np.asarray(self.successes, bool).reshape(n, -1))

    def state_dict(self) -> Dict:
        return dict(seed=self.seed, serial=self.serial, last_eval_timestep=self.last_eval_timestep,
                    last_mean_reward=self.last_mean_reward, best_mean_reward=self.best_mean_reward,
                    timesteps=list(self.timesteps), results=[list(r) for r in self.results],
                    ep_lengths=[list(r) for r in self.ep_lengths], successes=[list(r) for r in self.successes])

    def load_state_dict(self, d: Dict) -> None:
        self.seed, self.serial, self.last_eval_timestep = int(d["seed"]), int(d["serial"]), int(d["last_eval_timestep"])
        self.last_mean_reward, self.best_mean_reward = float(d["last_mean_reward"]), float(d["best_mean_reward"])
        self.timesteps = [int(t) for t in d["timesteps"]]
        self.results, self.ep_lengths = [list(r) for r in d["results"]], [list(r) for r in d["ep_lengths"]]
        self.successes = [list(r) for r in d["successes"]]
