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

from .dqn_train import check_ray_buffer
from .per_tree import _CPerParams
from .solver import MpcGpuError, bind_exports, load_library

_VP, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
# export -> (restype, argtypes); include/mpcgpu_dqn_per.h
_DQN_PER_TABLE = {
    # the second argument is an MpcGpuDqnParams*: the struct is dqn_fused's (which imports this module), passed by reference
    "mpcgpu_dqn_train_per_dev": (_I32, [_I32, _VP, C.POINTER(_CPerParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                        _I64, _I32, _I32, _U64, _U64, _VP, _VP, _VP, _VP]),
    "mpcgpu_dqn_per_last_error": (C.c_char_p, []),
}
DQN_PER_EXPORTS = tuple(_DQN_PER_TABLE)


def _bind(lib):
    return bind_exports(lib, "dqn_per", _DQN_PER_TABLE, "csrc/dqngpu.hip")


def check_buffer(trainer, buffer) -> None:
    """What the kernel assumes of a prioritized ray buffer on the trainer's device (``dqn_train.check_ray_buffer``, and that
    there is a tree at all); raises before anything is enqueued."""
    if getattr(buffer, "sum_tree", None) is None:
        raise ValueError("train_per() needs a prioritized buffer (ReplayBuffer(..., per_kwargs={...})); a uniform one goes to train()")
    check_ray_buffer(buffer, trainer.device)


def train_per(trainer, buffer, k: int, batch_size: int, indices: torch.Tensor = None, td: torch.Tensor = None) -> torch.Tensor:
    """``k`` gradient steps of ``trainer`` (a :class:`dqn_fused.FusedDqnTrainer`) on minibatches of ``batch_size`` rows drawn by
    priority from ``buffer`` by the kernel itself, through the trainer's launch loop and so with the contract of its ``train``:
    step s draws its uniforms from the counter stream ``(seed, serial + s)``, ``serial`` moves on by ``k``, the target network is
    not synchronised inside.  Returns the ``k`` losses (device).  ``indices`` (int64 ``[k, batch_size]``) and ``td`` (float32
    ``[k, batch_size]``), when given, take every step's tree indices and TD errors."""
    check_buffer(trainer, buffer)
    n = int(batch_size)
    for name, x, dtype in (("indices", indices, torch.int64), ("td", td, torch.float32)):
        if x is not None and (x.dtype != dtype or not x.is_contiguous() or x.device != trainer.device or x.numel() != k * max(n, 0)):
            raise ValueError(f"{name} must be {k} x {n} contiguous {dtype} values on {trainer.device}")
    lib, tree = _bind(load_library()), buffer.sum_tree

    def launch(part, done, losses):
        rc = lib.mpcgpu_dqn_train_per_dev(
            trainer.device_index, C.byref(trainer.params), C.byref(tree.params), trainer.state.data_ptr(), tree.tree.data_ptr(),
            buffer.obs.data_ptr(), buffer.next_obs.data_ptr(), buffer.actions.data_ptr(), buffer.rewards.data_ptr(),
            buffer.dones.data_ptr(), int(buffer.size), n, part, trainer.seed % 2 ** 64, trainer.serial % 2 ** 64, losses.data_ptr(),
            None if indices is None else indices.view(-1)[done * n:].data_ptr(),
            None if td is None else td.view(-1)[done * n:].data_ptr(), torch.cuda.current_stream(trainer.device).cuda_stream)
        if rc != 0:
            raise MpcGpuError(lib.mpcgpu_dqn_per_last_error().decode())
    return trainer.launch_steps(k, launch, "train_per")
