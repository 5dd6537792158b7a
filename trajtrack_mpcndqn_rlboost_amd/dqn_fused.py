"""Fused DQN update of the ray Q-network: host side of ``include/mpcgpu_dqn.h``.

:class:`FusedDqnTrainer` is a :class:`dqn_train.DqnTrainerBase` like :class:`dqn_train.DqnTrainer` -- the process group and
the update / target-sync counters are the base's, the surface :class:`dqn_train.DqnLearner` uses is the same -- but its
update is ONE launch of ``csrc/dqngpu.hip`` instead of ~40 torch kernels, and :meth:`FusedDqnTrainer.train` runs K updates
on a uniform replay buffer in one launch.  Parameters, target parameters, Adam moments and the step count live in one state
block on the device; ``q_net`` and ``q_net_target`` are real ``QNetwork`` modules whose parameters are views into it.
There is no fallback in torch operations: without the kernels the calls raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
import torch.distributed as dist

from . import dqn_per_fused
from .dqn import N_ACTIONS, OBS_DIM, QNetwork
from .dqn_train import DqnTrainerBase, check_ray_buffer
from .solver import MpcGpuError, bind_exports, load_library

N_PARAMS = 1177
MAX_ROWS = 256
MAX_STEPS = 65536
STATE_T = 4 * N_PARAMS
SHAPES = ((16, OBS_DIM), (16,), (16, 16), (16,), (N_ACTIONS, 16), (N_ACTIONS,))      # QNetwork.parameters()


class _CDqnParams(C.Structure):
    _fields_ = [("lr", C.c_double), ("gamma", C.c_double), ("max_grad_norm", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("double_q", C.c_int32), ("reserved", C.c_int32)]


_VP, _I32, _I64, _U64, _PP = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.POINTER(_CDqnParams)
_MINIBATCH = [_I32, _PP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP]
# export -> (restype, argtypes); include/mpcgpu_dqn.h
_DQN_TABLE = {
    "mpcgpu_dqn_state_floats": (_I32, []),
    "mpcgpu_dqn_grad_dev": (_I32, _MINIBATCH),
    "mpcgpu_dqn_apply_dev": (_I32, [_I32, _PP, _VP, _VP, C.c_float, _VP]),
    "mpcgpu_dqn_step_dev": (_I32, _MINIBATCH),
    "mpcgpu_dqn_train_dev": (_I32, [_I32, _PP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _U64, _U64, _VP, _VP]),
    "mpcgpu_dqn_last_error": (C.c_char_p, []),
}
DQN_EXPORTS = tuple(_DQN_TABLE)


def _bind(lib):
    return bind_exports(lib, "dqn", _DQN_TABLE, "csrc/dqngpu.hip")


def check_shape(q_net) -> None:
    shapes = tuple(tuple(p.shape) for p in q_net.parameters())
    if shapes != SHAPES:
        raise ValueError(f"the fused update is built for dqn.QNetwork's shape {SHAPES}, not {shapes}")


def adam_state_of(sd: Dict):
    """``torch.optim.Adam.state_dict()`` of a QNetwork -> (m [1177], v [1177], t) on the host; an empty state is t = 0."""
    ids = [i for g in sd["param_groups"] for i in g["params"]]
    if len(ids) != len(SHAPES):
        raise ValueError(f"optimizer checkpoint holds {len(ids)} parameters, the Q-network {len(SHAPES)}")
    m, v, steps = [], [], set()
    for i, shape in zip(ids, SHAPES):
        st = sd["state"].get(i)
        if st is None:
            m.append(torch.zeros(shape).reshape(-1)); v.append(torch.zeros(shape).reshape(-1)); steps.add(0)
            continue
        for k in ("exp_avg", "exp_avg_sq"):
            if tuple(torch.as_tensor(st[k]).shape) != shape:
                raise ValueError(f"optimizer checkpoint: {k} of parameter {i} has shape {tuple(torch.as_tensor(st[k]).shape)}, expected {shape}")
        m.append(torch.as_tensor(st["exp_avg"]).detach().float().cpu().reshape(-1))
        v.append(torch.as_tensor(st["exp_avg_sq"]).detach().float().cpu().reshape(-1))
        steps.add(int(float(torch.as_tensor(st["step"]))))
    if len(steps) != 1:
        raise ValueError(f"optimizer checkpoint: the parameters have different step counts {sorted(steps)}")
    return torch.cat(m), torch.cat(v), steps.pop()


def adam_groups(lr: float):
    """The parameter-group half of ``torch.optim.Adam.state_dict()`` for a QNetwork, from a real (never stepped) Adam."""
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in SHAPES], lr=lr).state_dict()["param_groups"]


def adam_state_dict(m: torch.Tensor, v: torch.Tensor, t: int, groups) -> Dict:
    """The reverse of :func:`adam_state_of`: flat moments [1177] and the step count -> the form ``torch.optim.Adam`` loads."""
    m, v = m.detach().cpu(), v.detach().cpu()
    state, off = {}, 0
    for i, shape in enumerate(SHAPES):
        n = 1
        for s in shape:
            n *= s
        state[i] = dict(step=torch.tensor(float(t)), exp_avg=m[off:off + n].reshape(shape).clone(),
                        exp_avg_sq=v[off:off + n].reshape(shape).clone())
        off += n
    return dict(state=state, param_groups=[dict(g) for g in groups])


class _AdamView:
    """What ``DqnLearner`` asks of ``trainer.optimizer``: the state in the form of ``torch.optim.Adam.state_dict()``."""

    def __init__(self, trainer: "FusedDqnTrainer"):
        self._tr = trainer

    def state_dict(self) -> Dict:
        tr = self._tr
        return adam_state_dict(tr.state[2 * N_PARAMS:3 * N_PARAMS], tr.state[3 * N_PARAMS:4 * N_PARAMS], tr.step_count, tr._groups)

    def load_state_dict(self, sd: Dict) -> None:
        self._tr.load_optimizer_state(sd)


class FusedDqnTrainer(DqnTrainerBase):
    def __init__(self, q_net: Optional[QNetwork] = None, lr: float = 1e-4, gamma: float = 0.98,
                 target_update_interval: int = 10_000, max_grad_norm: float = 10.0, double_q: bool = False,
                 device: str = "cuda", force_collective: bool = False, seed: int = 0):
        src = q_net if q_net is not None else QNetwork()
        check_shape(src)
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise MpcGpuError(f"FusedDqnTrainer needs a HIP device (got device {str(device)!r}, torch.cuda.is_available() = "
                              f"{torch.cuda.is_available()}); there is no CPU path -- use DqnTrainer")
        self.device_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self.device_index)
        self._lib = _bind(load_library())
        super().__init__(target_update_interval, force_collective)
        self.state = torch.zeros(self._lib.mpcgpu_dqn_state_floats(), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            self.state[:N_PARAMS] = torch.cat([p.detach().reshape(-1).float() for p in src.parameters()]).to(self.device)
            if self.world > 1:       # replicas must START equal: rank 0's weights win
                dist.broadcast(self.state[:N_PARAMS], src=0)
            self.state[N_PARAMS:2 * N_PARAMS] = self.state[:N_PARAMS]
        self.q_net = self._view_network(0, True)
        self.q_net_target = self._view_network(N_PARAMS, False)
        self._t = self.state[STATE_T:STATE_T + 2].view(torch.int64)
        self.params = _CDqnParams(float(lr), float(gamma), float(max_grad_norm), 0.9, 0.999, 1e-8, int(bool(double_q)), 0)
        self._groups = adam_groups(lr)
        self.optimizer = _AdamView(self)
        self.gamma, self.max_grad_norm, self.double_q = gamma, max_grad_norm, bool(double_q)
        self.seed, self.serial = int(seed), 0           # the sample stream of train(): step s draws from (seed, serial + s)
        self._bucket = torch.zeros(N_PARAMS, dtype=torch.float32, device=self.device)     # the gradient, and the all-reduce bucket
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._td = torch.zeros(MAX_ROWS, dtype=torch.float32, device=self.device)
        self.last_td_error = self._td[:0]

    def _view_network(self, offset: int, requires_grad: bool) -> QNetwork:
        net = QNetwork()
        for p, shape in zip(net.parameters(), SHAPES):
            n = p.numel()
            p.data = self.state[offset:offset + n].view(shape)
            offset += n
        return net.requires_grad_(requires_grad)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise MpcGpuError(self._lib.mpcgpu_dqn_last_error().decode())

    @property
    def step_count(self) -> int:
        """Adam's t (reading it synchronises)."""
        return int(self._t[0])

    def _minibatch(self, batch: Dict[str, torch.Tensor]):
        f32 = lambda x: x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        obs, next_obs = f32(batch["obs"]), f32(batch["next_obs"])
        n = obs.shape[0]
        if obs.dim() != 2 or obs.shape[1] != OBS_DIM or next_obs.shape != obs.shape:
            raise ValueError(f"obs and next_obs must be [n, {OBS_DIM}], got {tuple(obs.shape)} and {tuple(next_obs.shape)}")
        actions = batch["actions"].to(device=self.device, dtype=torch.int64).contiguous()
        rewards, dones = f32(batch["rewards"]).reshape(-1), f32(batch["dones"]).reshape(-1)
        weights = f32(batch["weights"]).reshape(-1) if "weights" in batch else None
        for name, x in (("actions", actions), ("rewards", rewards), ("dones", dones), ("weights", weights)):
            if x is not None and x.numel() != n:
                raise ValueError(f"{name} has {x.numel()} entries for {n} rows")
        keep = (obs, next_obs, actions, rewards, dones, weights)
        return keep, n, (obs.data_ptr(), next_obs.data_ptr(), actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(),
                         weights.data_ptr() if weights is not None else None)

    def _call(self, fn, batch):
        keep, n, ptrs = self._minibatch(batch)
        self._check(fn(self.device_index, C.byref(self.params), self.state.data_ptr(), *ptrs, n, self._bucket.data_ptr(),
                       self._loss.data_ptr(), self._td.data_ptr(), self._stream()))
        self.last_td_error = self._td[:n]
        return keep

    def grad(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """The unclipped mean gradient of ``batch`` into the bucket (returned); loss and TD errors as ``update`` leaves them."""
        self._call(self._lib.mpcgpu_dqn_grad_dev, batch)
        return self._bucket

    def apply(self, grad: torch.Tensor, scale: float = 1.0) -> None:
        """Clip, Adam step, t += 1 with ``grad * scale``."""
        if grad.numel() != N_PARAMS or grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != self.device:
            raise ValueError(f"the gradient is {N_PARAMS} contiguous float32 values on {self.device}")
        self._check(self._lib.mpcgpu_dqn_apply_dev(self.device_index, C.byref(self.params), self.state.data_ptr(), grad.data_ptr(),
                                                   float(scale), self._stream()))

    def update(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """One gradient step on ``batch`` (the keys of ``DqnTrainer.update``, at most 256 rows).  Returns the loss as a device
        tensor; ``last_td_error`` [n] holds the TD errors.  One rank: one launch.  Several ranks (or ``force_collective``):
        the gradient kernel into the bucket, ONE all-reduce, the apply kernel with scale 1 / world."""
        if self._collective:
            self.grad(batch)
            dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM)
            self.apply(self._bucket, 1.0 / self.world)
        else:
            self._call(self._lib.mpcgpu_dqn_step_dev, batch)
        self._count_updates()
        return self._loss[0]

    def theta(self) -> torch.Tensor:
        return self.state           # the state block begins with theta: no copy

    def launch_steps(self, k: int, launch, name: str = "train") -> torch.Tensor:
        """The K-step launch loop of :meth:`train` and :meth:`train_per`: ``k`` steps in launches of at most 65 536.
        ``launch(part, done, losses)`` enqueues steps ``done .. done + part - 1`` on the stream ``(seed, serial)`` and raises on a
        refusal; ``serial`` moves on and the updates are counted.  Returns the ``k`` losses (device)."""
        if self._collective:
            raise MpcGpuError(f"{name}() is the one-rank path; several ranks update step by step around the all-reduce")
        if k < 1:
            raise ValueError(f"k = {k}: at least one step")
        losses = torch.empty(k, dtype=torch.float32, device=self.device)
        done = 0
        while done < k:
            part = min(k - done, MAX_STEPS)
            launch(part, done, losses[done:])
            self.serial += part
            self._count_updates(part, sync=False)
            done += part
        return losses

    def train(self, buffer, k: int, batch_size: int) -> torch.Tensor:
        """``k`` gradient steps on minibatches of ``batch_size`` rows drawn uniformly from ``buffer`` (a
        ``dqn_train.ReplayBuffer``) by the kernel itself, 65 536 steps per launch: step s draws from the counter stream
        ``(seed, serial + s)``, and ``serial`` moves on by ``k``.  Returns the ``k`` losses (device).  The target network is
        not synchronised inside (``target_update_interval`` does not apply): the learner syncs on environment steps."""
        check_ray_buffer(buffer, self.device)
        return self.launch_steps(k, lambda part, done, losses: self._check(self._lib.mpcgpu_dqn_train_dev(
            self.device_index, C.byref(self.params), self.state.data_ptr(), buffer.obs.data_ptr(), buffer.next_obs.data_ptr(),
            buffer.actions.data_ptr(), buffer.rewards.data_ptr(), buffer.dones.data_ptr(), int(buffer.size), int(batch_size),
            part, self.seed % 2 ** 64, self.serial % 2 ** 64, losses.data_ptr(), self._stream())))

    def train_per(self, buffer, k: int, batch_size: int) -> torch.Tensor:
        """:meth:`train` on a PRIORITIZED buffer: sample from its sum tree, weighted step, priorities written back, ``k`` times
        in one launch (:func:`dqn_per_fused.train_per`)."""
        return dqn_per_fused.train_per(self, buffer, k, batch_size)

    def sync_target(self) -> None:
        """Hard target update: a copy of 1 177 floats inside the state block."""
        with torch.no_grad():
            self.state[N_PARAMS:2 * N_PARAMS].copy_(self.state[:N_PARAMS])
        self.num_target_syncs += 1

    def load_optimizer_state(self, sd: Dict) -> None:
        """Adam's moments and step count from the form of ``torch.optim.Adam.state_dict()``; checked before anything is written."""
        m, v, t = adam_state_of(sd)
        for key, mine in (("lr", self.params.lr), ("betas", (self.params.beta1, self.params.beta2)), ("eps", self.params.eps)):
            for g in sd["param_groups"]:
                if key in g:
                    theirs = tuple(g[key]) if isinstance(g[key], (tuple, list)) else g[key]
                    if theirs != mine:
                        raise ValueError(f"optimizer checkpoint has {key} = {theirs!r}, this trainer {mine!r}")
        with torch.no_grad():
            self.state[2 * N_PARAMS:3 * N_PARAMS] = m.to(self.device)
            self.state[3 * N_PARAMS:4 * N_PARAMS] = v.to(self.device)
            self._t.fill_(t)

