"""Prioritized replay inside the fused DQN launch: host side of ``include/mpcgpu_dqn_per.h``.

:func:`train_per` runs K gradient steps of a :class:`dqn_fused.FusedDqnTrainer` on a prioritized
:class:`dqn_train.ReplayBuffer` in ONE launch of ``csrc/dqngpu.hip``: every step draws its minibatch from the buffer's sum tree,
makes the weighted update and writes the new priorities back before the next step samples -- bit for bit what
``SumTree.sample``, ``FusedDqnTrainer.update`` and ``SumTree.update`` do in K rounds, without the launches around them.
There is no fallback in torch operations: without the kernel the call raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from .dqn import OBS_DIM
from .dqn_fused import MAX_STEPS, _CDqnParams
from .per_tree import _CPerParams
from .solver import MpcGpuError, bind_exports

_VP, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
# export -> (restype, argtypes); include/mpcgpu_dqn_per.h
_DQN_PER_TABLE = {
    "mpcgpu_dqn_train_per_dev": (_I32, [_I32, C.POINTER(_CDqnParams), C.POINTER(_CPerParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                        _I64, _I32, _I32, _U64, _U64, _VP, _VP, _VP, _VP]),
    "mpcgpu_dqn_per_last_error": (C.c_char_p, []),
}
DQN_PER_EXPORTS = tuple(_DQN_PER_TABLE)


def _bind(lib):
    return bind_exports(lib, "dqn_per", _DQN_PER_TABLE, "csrc/dqngpu.hip")


def check_buffer(trainer, buffer) -> None:
    """What the kernel assumes of a prioritized ray buffer on the trainer's device; raises before anything is enqueued."""
    tree = getattr(buffer, "sum_tree", None)
    if tree is None:
        raise ValueError("train_per() needs a prioritized buffer (ReplayBuffer(..., per_kwargs={...})); a uniform one goes to train()")
    for name, dtype in (("obs", torch.float32), ("next_obs", torch.float32), ("actions", torch.int64),
                        ("rewards", torch.float32), ("dones", torch.float32)):
        x = getattr(buffer, name)
        if x.dtype != dtype or not x.is_contiguous() or x.device != trainer.device:
            raise ValueError(f"buffer.{name} must be contiguous {dtype} on {trainer.device}")
        if x.shape[0] != tree.capacity:
            raise ValueError(f"buffer.{name} holds {x.shape[0]} rows, the tree's capacity is {tree.capacity}")
    if buffer.obs.shape[1:] != (OBS_DIM,):
        raise ValueError(f"the buffer holds observations of shape {tuple(buffer.obs.shape[1:])}, not ({OBS_DIM},)")
    t = tree.tree
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != trainer.device or t.numel() != 2 * tree.capacity - 1:
        raise ValueError(f"the sum tree must be {2 * tree.capacity - 1} contiguous float64 values on {trainer.device}")


def train_per(trainer, buffer, k: int, batch_size: int, indices: torch.Tensor = None, td: torch.Tensor = None) -> torch.Tensor:
    """``k`` gradient steps of ``trainer`` on minibatches of ``batch_size`` rows drawn by priority from ``buffer`` by the kernel
    itself, 65 536 steps per launch; the contract of ``FusedDqnTrainer.train``: step s draws its uniforms from the counter
    stream ``(seed, serial + s)``, ``serial`` moves on by ``k``, the target network is not synchronised inside.  Returns the
    ``k`` losses (device).  ``indices`` (int64 ``[k, batch_size]``) and ``td`` (float32 ``[k, batch_size]``), when given, take
    every step's tree indices and TD errors."""
    if trainer.collective:
        raise MpcGpuError("train_per() is the one-rank path; several ranks update step by step around the all-reduce")
    if k < 1:
        raise ValueError(f"k = {k}: at least one step")
    check_buffer(trainer, buffer)
    n = int(batch_size)
    for name, x, dtype in (("indices", indices, torch.int64), ("td", td, torch.float32)):
        if x is not None and (x.dtype != dtype or not x.is_contiguous() or x.device != trainer.device or x.numel() != k * max(n, 0)):
            raise ValueError(f"{name} must be {k} x {n} contiguous {dtype} values on {trainer.device}")
    lib, tree = _bind(trainer._lib), buffer.sum_tree
    losses = torch.empty(k, dtype=torch.float32, device=trainer.device)
    done = 0
    while done < k:
        part = min(k - done, MAX_STEPS)
        rc = lib.mpcgpu_dqn_train_per_dev(
            trainer.device_index, C.byref(trainer.params), C.byref(tree.params), trainer.state.data_ptr(), tree.tree.data_ptr(),
            buffer.obs.data_ptr(), buffer.next_obs.data_ptr(), buffer.actions.data_ptr(), buffer.rewards.data_ptr(),
            buffer.dones.data_ptr(), int(buffer.size), n, part, trainer.seed % 2 ** 64, trainer.serial % 2 ** 64,
            losses[done:].data_ptr(), None if indices is None else indices.view(-1)[done * n:].data_ptr(),
            None if td is None else td.view(-1)[done * n:].data_ptr(), trainer._stream())
        if rc != 0:
            raise MpcGpuError(lib.mpcgpu_dqn_per_last_error().decode())
        trainer.serial += part
        trainer._count_updates(part, sync=False)
        done += part
    return losses
