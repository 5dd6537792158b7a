"""Device-resident sum tree of prioritized experience replay: host side of ``include/mpcgpu_per.h``.

The tree and its state block are torch tensors on the environment's device; every method enqueues HIP kernels of
``csrc/pergpu.hip`` on torch's current stream and returns -- nothing here synchronises with the host.  There is no
fallback in torch operations: without the kernels the calls raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch

from .solver import MpcGpuError, bind_exports, load_library

MAX_ROWS = 4096


class _CPerParams(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("update_max_freq", C.c_int64), ("alpha", C.c_double), ("beta", C.c_double),
                ("epsilon", C.c_double), ("initial_priority", C.c_double)]


_VP, _I32, _I64, _PP = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(_CPerParams)
# export -> (restype, argtypes); include/mpcgpu_per.h
_PER_TABLE = {
    "mpcgpu_per_state_doubles": (_I32, []),
    "mpcgpu_per_reset_dev": (_I32, [_I32, _PP, _VP, _VP, _VP]),
    "mpcgpu_per_add_dev": (_I32, [_I32, _PP, _VP, _VP, _I64, _I64, _I64, _VP]),
    "mpcgpu_per_update_dev": (_I32, [_I32, _PP, _VP, _VP, _VP, _I32, _VP]),
    "mpcgpu_per_sample_dev": (_I32, [_I32, _PP, _VP, _VP, _I32, _I64, _VP, _VP, _VP, _VP]),
    "mpcgpu_per_stats_dev": (_I32, [_I32, _PP, _VP, _VP, _VP, _VP]),
    "mpcgpu_per_last_error": (C.c_char_p, []),
}
PER_EXPORTS = tuple(_PER_TABLE)


def _bind(lib):
    return bind_exports(lib, "per", _PER_TABLE, "csrc/pergpu.hip")


class SumTree:
    """``tree``: float64 [2 capacity - 1], heap order, leaf of ring position ``p`` at ``p + capacity - 1``;
    ``state``: float64 state block (max_p, rows since max_p was read, ...)."""

    def __init__(self, capacity: int, device, alpha: float = 0.3, beta: float = 0.4, epsilon: float = 1e-3,
                 update_max_freq: int = 1_000, initial_priority: float = 1.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise MpcGpuError("the sum tree lives on the GPU (there is no CPU path)")
        self.device_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._lib = _bind(load_library())
        self.capacity = int(capacity)
        self.params = _CPerParams(self.capacity, int(update_max_freq), float(alpha), float(beta), float(epsilon),
                                  float(initial_priority))
        self.tree = torch.zeros(2 * self.capacity - 1, dtype=torch.float64, device=self.device)
        self.state = torch.zeros(self._lib.mpcgpu_per_state_doubles(), dtype=torch.float64, device=self.device)
        self.reset()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise MpcGpuError(self._lib.mpcgpu_per_last_error().decode())

    def reset(self) -> None:
        self._check(self._lib.mpcgpu_per_reset_dev(self.device_index, C.byref(self.params), self.tree.data_ptr(),
                                                   self.state.data_ptr(), self._stream()))

    def add(self, pos: int, n: int, n_entries: int) -> None:
        """Rows ``pos .. pos + n - 1`` (mod capacity) take max_p; ``n_entries`` = rows stored before this call."""
        self._check(self._lib.mpcgpu_per_add_dev(self.device_index, C.byref(self.params), self.tree.data_ptr(),
                                                 self.state.data_ptr(), int(pos), int(n), int(n_entries), self._stream()))

    def update(self, indices: torch.Tensor, td_error: torch.Tensor) -> None:
        """Leaf ``indices[i]`` takes ``(|td_error[i]| + epsilon)^alpha``; on a repeated index the highest row wins."""
        indices = indices.to(device=self.device, dtype=torch.int64).contiguous()
        td_error = td_error.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if indices.numel() != td_error.numel():
            raise ValueError(f"{indices.numel()} indices but {td_error.numel()} TD errors")
        self._check(self._lib.mpcgpu_per_update_dev(self.device_index, C.byref(self.params), self.tree.data_ptr(),
                                                    indices.data_ptr(), td_error.data_ptr(), indices.numel(), self._stream()))

    def sample(self, u: torch.Tensor, n_entries: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``u``: float64 uniforms in [0, 1), one per row -> (tree indices int64, ring positions int64, weights float32)."""
        u = u.to(device=self.device, dtype=torch.float64).contiguous()
        n = u.numel()
        indices = torch.empty(n, dtype=torch.int64, device=self.device)
        positions = torch.empty(n, dtype=torch.int64, device=self.device)
        weights = torch.empty(n, dtype=torch.float32, device=self.device)
        self._check(self._lib.mpcgpu_per_sample_dev(self.device_index, C.byref(self.params), self.tree.data_ptr(), u.data_ptr(),
                                                    n, int(n_entries), indices.data_ptr(), positions.data_ptr(),
                                                    weights.data_ptr(), self._stream()))
        return indices, positions, weights

    def stats(self) -> torch.Tensor:
        """Device tensor (sum of all priorities, max_p): diagnostics, reading it on the host synchronises."""
        out = torch.empty(2, dtype=torch.float64, device=self.device)
        self._check(self._lib.mpcgpu_per_stats_dev(self.device_index, C.byref(self.params), self.tree.data_ptr(),
                                                   self.state.data_ptr(), out.data_ptr(), self._stream()))
        return out

    # ---- checkpoint: the leaves and the head of the state block; inner nodes are sums of their children and are rebuilt
    def state_dict(self, n_entries: int):
        C0 = self.capacity - 1
        return dict(leaves=self.tree[C0:C0 + n_entries].clone(), state=self.state[:4].clone())

    def load_state_dict(self, src) -> None:
        leaves = src["leaves"].to(self.device)
        if leaves.numel() > self.capacity:
            raise ValueError(f"checkpointed tree holds {leaves.numel()} leaves, this tree only {self.capacity}")
        self.tree.zero_()
        self.state.zero_()
        self.state[:4] = src["state"].to(self.device)
        C0 = self.capacity - 1
        self.tree[C0:C0 + leaves.numel()] = leaves
        # restore path (once per run, not the hot path): every inner node from its children, depth by depth, deepest first
        depth = (2 * self.capacity - 1).bit_length() - 1
        for d in range(depth - 1, -1, -1):
            lo, hi = (1 << d) - 1, min((1 << (d + 1)) - 2, C0 - 1)
            if hi >= lo:
                self.tree[lo:hi + 1] = self.tree[2 * lo + 1:2 * hi + 2:2] + self.tree[2 * lo + 2:2 * hi + 3:2]
