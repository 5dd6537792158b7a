"""Collection inside one launch on the two-record table: host side of ``include/mpcgpu_collect_fresh.h``.

:func:`collect_rays_fresh` is :func:`collect.collect_rays` for a :class:`rl_env.BatchedRaysEnv` after ``enable_spares()`` /
``enable_fresh_maps()``: T steps -- act, auto-reset step WITH map turnover, ring row, episode return -- in ONE launch of
``csrc/envgpu.hip``, bit for bit what :func:`collect.act`, the fresh-map step (auto-reset, no refill between the rounds) and
``ReplayBuffer.add`` do in T rounds.  The argument checks and the bookkeeping behind the launch are those of ``collect.py``.
There is no fallback in torch operations: without the kernel the call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import collect
from .rl_env import _CParams
from .solver import MpcGpuError, bind_exports

_VP, _I32 = C.c_void_p, C.c_int32
# export -> (restype, argtypes); include/mpcgpu_collect_fresh.h
_COLLECT_FRESH_TABLE = {
    "mpcgpu_collect_rays_fresh_dev": (_I32, [_I32, C.POINTER(_CParams), _I32] + [_VP] * 13
                                      + [_I32, _VP, C.POINTER(collect._CCollectParams)] + [_VP] * 11),
    "mpcgpu_collect_fresh_last_error": (C.c_char_p, []),
}
COLLECT_FRESH_EXPORTS = tuple(_COLLECT_FRESH_TABLE)
# steps per launch ``DqnLearner(collect_turnover=True)`` defaults to: the largest of 4, 16, 64 without a stale reset in 2000 steps
# of random actions at B = 4096 with refill_every 16 (profiles/collect_fresh_bench.txt, the rule of enable_fresh_maps)
DEFAULT_LAUNCH_STEPS = 16


def _bind(lib):
    return bind_exports(lib, "collect_fresh", _COLLECT_FRESH_TABLE, "csrc/envgpu.hip")


def check_env(env) -> None:
    """What the kernel is built for: the ray environment on the two-record table.  Raises ``ValueError`` otherwise."""
    if getattr(env, "is_image_env", False):
        raise ValueError("collection inside the launch is built for the ray environment only: the image environment's "
                         "observation is drawn by a second kernel")
    if getattr(env, "records2", None) is None:
        raise ValueError("collect_rays_fresh runs on the two-record table: call enable_spares() or enable_fresh_maps() on the "
                         "environment first (collect.collect_rays is the entry for one record table)")


def collect_rays_fresh(env, theta: torch.Tensor, buffer, eps: Sequence[float], seed: int, serial: int, ep_return: torch.Tensor,
                       out: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """:func:`collect.collect_rays` -- the same arguments, ring bookkeeping and sum-tree adds behind the launch -- on an
    environment after ``enable_spares()`` / ``enable_fresh_maps()``: a row whose episode ends inside the launch while its spare
    is ready starts the next episode on the spare (``loaded``), a row without a ready spare resets on the map it is on
    (``stale``).  There is one spare per row and no refill inside a launch, so only the FIRST ending of a row in a launch can
    turn over; every later one counts as stale.

    A launch of T steps equals T rounds of ``collect.act`` and ``env.step(actions, auto_reset=True)`` WITHOUT a refill between
    them.  With ``enable_fresh_maps(refill_every=R)`` the T steps are counted behind the launch and at most ONE refill is
    enqueued there, if a multiple of R was passed.  So a run in launches equals the host-driven run only where every refill
    point falls on the end of a launch; otherwise the refill comes later than the host-driven loop would enqueue it and a
    row may go stale that would not have."""
    check_env(env)
    args = collect.rays_args(env, theta, buffer, eps, seed, serial, ep_return, out)
    lib = _bind(env._lib)
    rc = lib.mpcgpu_collect_rays_fresh_dev(env.device_index, C.byref(env.params), env.B, env.records2.data_ptr(),
                                           env.which.data_ptr(), env.spare_ready.data_ptr(), env.loaded.data_ptr(),
                                           env.stale.data_ptr(), *args)
    if rc != 0:
        raise MpcGpuError(lib.mpcgpu_collect_fresh_last_error().decode())
    collect.ring_moved(buffer, len(eps), env.B)
    env._count_autoreset_steps(len(eps))
