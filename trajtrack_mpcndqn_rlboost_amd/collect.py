"""Collection inside one launch: host side of ``include/mpcgpu_collect.h``.

:func:`collect_rays` runs T steps of a :class:`rl_env.BatchedRaysEnv` in ONE launch of ``csrc/envgpu.hip``: every step the
wavefront of a row evaluates the ray Q-network on the observation the environment holds, draws its epsilon-greedy action from
the counter stream ``(seed, serial + t)``, makes the auto-reset step and writes the transition into the replay buffer's ring --
bit for bit what :func:`act`, ``env.step(auto_reset=True)`` and ``ReplayBuffer.add`` do in T rounds, without the launches around
them.  :func:`act` is the action rule alone.  There is no fallback in torch operations: without the kernels the calls raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from .dqn import N_ACTIONS, OBS_DIM
from .dqn_fused import N_PARAMS
from .dqn_train import check_ray_buffer
from .rl_env import N_EXTERNAL, N_INTERNAL, _CParams
from .solver import MpcGpuError, bind_exports, load_library

MAX_STEPS = 64
OUTPUTS = (("actions", torch.int32), ("done", torch.uint8), ("success", torch.uint8), ("episode_return", torch.float64))


class _CCollectParams(C.Structure):
    _fields_ = [("eps", C.c_double * MAX_STEPS), ("seed", C.c_uint64), ("serial0", C.c_uint64), ("capacity", C.c_int64),
                ("pos0", C.c_int64), ("T", C.c_int32), ("reserved", C.c_int32)]


_VP, _I32, _U64 = C.c_void_p, C.c_int32, C.c_uint64
# export -> (restype, argtypes); include/mpcgpu_collect.h
_COLLECT_TABLE = {
    "mpcgpu_collect_act_dev": (_I32, [_I32, _VP, _VP, _VP, _I32, C.c_double, _U64, _U64, _VP, _VP, _VP]),
    "mpcgpu_collect_rays_dev": (_I32, [_I32, C.POINTER(_CParams), _I32] + [_VP] * 9 + [_I32, _VP, C.POINTER(_CCollectParams)]
                                + [_VP] * 11),
    "mpcgpu_collect_last_error": (C.c_char_p, []),
}
COLLECT_EXPORTS = tuple(_COLLECT_TABLE)


def _bind(lib):
    return bind_exports(lib, "collect", _COLLECT_TABLE, "csrc/envgpu.hip")


def check_env(env) -> None:
    """What the kernel is built for: the ray environment on one record table.  Raises ``ValueError`` otherwise."""
    if getattr(env, "is_image_env", False):
        raise ValueError("collection inside the launch is built for the ray environment only: the image environment's "
                         "observation is drawn by a second kernel")
    if getattr(env, "records2", None) is not None:
        raise ValueError("collection inside the launch is not built for an environment after enable_spares() / "
                         "enable_fresh_maps(): its step runs on the two-record table")


def _theta(theta: torch.Tensor, device) -> torch.Tensor:
    if (not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 or theta.dim() != 1 or theta.numel() < N_PARAMS
            or not theta.is_contiguous() or theta.device != device):
        raise ValueError(f"theta must be at least {N_PARAMS} contiguous float32 values on {device} (the layout of mpcgpu_dqn.h)")
    return theta


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise MpcGpuError(lib.mpcgpu_collect_last_error().decode())


def act(env_or_obs, theta: torch.Tensor, eps: float, seed: int, serial: int, return_q: bool = False):
    """The action rule of ``include/mpcgpu_collect.h`` on B rows in one launch -> ``actions`` int32 [B] (and ``q`` float32
    [B, 9] with ``return_q``).  ``env_or_obs``: a ray environment (the observation it holds), an observation dictionary
    (``external`` [B, 32], ``internal`` [B, 14]) or the flat [B, 46] tensor of ``flatten_observation``."""
    if isinstance(env_or_obs, torch.Tensor):
        if env_or_obs.dim() != 2 or env_or_obs.shape[1] != OBS_DIM:
            raise ValueError(f"a flat observation is [B, {OBS_DIM}], got {tuple(env_or_obs.shape)}")
        ext, inte = env_or_obs[:, :N_EXTERNAL], env_or_obs[:, N_EXTERNAL:]
    elif isinstance(env_or_obs, dict):
        ext, inte = env_or_obs["external"], env_or_obs["internal"]
    else:
        check_env(env_or_obs)
        ext, inte = env_or_obs.obs_external, env_or_obs.obs_internal
    device = ext.device
    if device.type != "cuda":
        raise MpcGpuError("collect.act needs a HIP device: the policy is a GPU kernel, there is no CPU path")
    ext, inte = ext.to(torch.float32).contiguous(), inte.to(device=device, dtype=torch.float32).contiguous()
    B = ext.shape[0]
    if ext.shape != (B, N_EXTERNAL) or inte.shape != (B, N_INTERNAL):
        raise ValueError(f"observations must be [B, {N_EXTERNAL}] and [B, {N_INTERNAL}], got {tuple(ext.shape)} and {tuple(inte.shape)}")
    theta = _theta(theta, device)
    lib = _bind(load_library())
    actions = torch.empty(B, dtype=torch.int32, device=device)
    q = torch.empty(B, N_ACTIONS, dtype=torch.float32, device=device) if return_q else None
    _check(lib, lib.mpcgpu_collect_act_dev(device.index, theta.data_ptr(), ext.data_ptr(), inte.data_ptr(), B, float(eps),
                                           int(seed) % 2 ** 64, int(serial) % 2 ** 64, actions.data_ptr(),
                                           None if q is None else q.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    return (actions, q) if return_q else actions


def rays_args(env, theta: torch.Tensor, buffer, eps: Sequence[float], seed: int, serial: int, ep_return: torch.Tensor,
              out: Optional[Dict[str, torch.Tensor]]) -> tuple:
    """The argument checks the T-step entries share (:func:`collect_rays`, ``collect_fresh.collect_rays_fresh``) -> the
    arguments of either entry from ``state`` on, the stream included.  ``ValueError`` before anything is enqueued."""
    T, B = len(eps), env.B
    device = env.device
    theta = _theta(theta, device)
    check_ray_buffer(buffer, device)
    if ep_return.dtype != torch.float64 or ep_return.shape != (B,) or not ep_return.is_contiguous() or ep_return.device != device:
        raise ValueError(f"ep_return must be {B} contiguous float64 values on {device}")
    ptr = {}
    for name, dtype in OUTPUTS:
        x = None if out is None else out.get(name)
        if x is not None and (x.dtype != dtype or not x.is_contiguous() or x.device != device or x.numel() != T * B):
            raise ValueError(f"out[{name!r}] must be {T} x {B} contiguous {dtype} values on {device}")
        ptr[name] = None if x is None else x.data_ptr()
    p = _CCollectParams(seed=int(seed) % 2 ** 64, serial0=int(serial) % 2 ** 64, capacity=int(buffer.capacity),
                        pos0=int(buffer.pos), T=T if T <= MAX_STEPS else MAX_STEPS + 1)
    for t, e in enumerate(eps[:MAX_STEPS]):
        p.eps[t] = float(e)
    return (env.state.data_ptr(), env.obs_internal.data_ptr(),
            env.obs_external.data_ptr(), env.reward.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
            env.term_internal.data_ptr(), env.term_external.data_ptr(), int(env.max_episode_steps), theta.data_ptr(), C.byref(p),
            buffer.obs.data_ptr(), buffer.next_obs.data_ptr(), buffer.actions.data_ptr(), buffer.rewards.data_ptr(),
            buffer.dones.data_ptr(), ep_return.data_ptr(), ptr["actions"], ptr["done"], ptr["success"], ptr["episode_return"],
            torch.cuda.current_stream(device).cuda_stream)


def ring_moved(buffer, T: int, B: int) -> None:
    """Behind a launch of T steps: ``buffer.pos`` and ``buffer.size`` as T calls of ``add`` move them, and with a sum tree its
    T calls of ``add``, one per step and in order."""
    for _ in range(T):
        if buffer.sum_tree is not None:
            buffer.sum_tree.add(buffer.pos, B, buffer.size)      # the new rows take the running maximum priority
        buffer.pos, buffer.size = (buffer.pos + B) % buffer.capacity, min(buffer.size + B, buffer.capacity)


def collect_rays(env, theta: torch.Tensor, buffer, eps: Sequence[float], seed: int, serial: int, ep_return: torch.Tensor,
                 out: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """``len(eps)`` steps (1 .. 64) of ``env`` in ONE launch: step t acts on the observation the environment holds with
    ``eps[t]`` and the counter stream ``(seed, serial + t)``, steps with auto-reset and writes its B transitions into
    ``buffer`` (a uniform or prioritized ``dqn_train.ReplayBuffer`` of flat observations) from ``buffer.pos`` on.
    ``ep_return`` [B] float64 is the running return per row, updated in place.  ``out`` may hold ``[T, B]`` tensors
    ``actions`` (int32), ``done``, ``success`` (uint8) and ``episode_return`` (float64, written where ``done``).

    ``buffer.pos`` and ``buffer.size`` move on as T calls of ``add`` would move them; with a sum tree those T calls of
    ``sum_tree.add`` follow the launch, one per step and in order (the tree's add counter and its maximum depend on the
    number of calls).  Refusals come before anything is enqueued and leave every tensor as it was.  An environment after
    ``enable_spares()`` is refused here: ``collect_fresh.collect_rays_fresh`` is its entry."""
    check_env(env)
    args = rays_args(env, theta, buffer, eps, seed, serial, ep_return, out)
    lib = _bind(env._lib)
    _check(lib, lib.mpcgpu_collect_rays_dev(env.device_index, C.byref(env.params), env.B, env.records.data_ptr(), *args))
    ring_moved(buffer, len(eps), env.B)
