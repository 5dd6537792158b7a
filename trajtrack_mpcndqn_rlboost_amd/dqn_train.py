"""Data-parallel DQN update for the action-value head (BASELINE.json config 5).

Hyper-parameters are the reference's SB3 settings (``src/test_block_rl.py:77-86`` and the ``data`` member of
``Model/ray/best_model.zip``): Huber loss, Adam lr 1e-4, gamma 0.98, batch 32, target sync every 10 000 steps,
gradient clip 10.  The reference trains a vanilla DQN in one process; this build adds (a) an optional Double-DQN
target (``double_q``; off by default = reference semantics) and (b) data parallelism: every rank computes the
gradient of its shard of the batch, ONE all-reduce of a single flat bucket of 1 177 fp32 values sums them
(RCCL over xGMI on MI355X -- 4.7 KB, pure latency), then every rank applies the same optimiser step.
"""
from __future__ import annotations

import copy
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist
from torch import nn
from torch.nn import functional as F

from .dqn import OBS_DIM, ImageQNetwork, QNetwork
from .per_tree import SumTree


class DqnTrainerBase:
    """What :class:`DqnTrainer` and :class:`dqn_fused.FusedDqnTrainer` share: the process group (``world``, ``collective``) and
    the update / target-sync counters.  The rest of what :class:`DqnLearner` uses -- ``q_net``, ``q_net_target``, ``optimizer``,
    ``update``, ``last_td_error``, ``sync_target``, ``load_optimizer_state``, ``theta`` -- is each class's own."""

    def __init__(self, target_update_interval: int, force_collective: bool = False):
        """``force_collective``: all-reduce the gradient (and run what is built around that) in a process group of ONE rank
        too -- the multi-rank code path, collective included, on a single GPU (tests)."""
        grouped = dist.is_available() and dist.is_initialized()
        if force_collective and not grouped:
            raise RuntimeError("force_collective needs an initialised process group")
        self.world = dist.get_world_size() if grouped else 1
        self._collective = self.world > 1 or force_collective
        self.target_update_interval, self.num_updates, self.num_target_syncs = target_update_interval, 0, 0

    collective = property(lambda self: self._collective, doc="Whether an update all-reduces its gradient (read-only).")

    def _count_updates(self, n: int = 1, sync: bool = True) -> None:
        """``n`` updates were made: count them and, with ``sync``, apply ``target_update_interval``."""
        self.num_updates += n
        if sync and self.target_update_interval and self.num_updates % self.target_update_interval == 0:
            self.sync_target()

    def theta(self) -> torch.Tensor:
        """The online parameters of a ray Q-network as the kernels read them (``collect.collect_rays``): at least 1 177
        contiguous float32 values on the device, ``QNetwork.parameters()`` in order at the front."""
        raise NotImplementedError


class DqnTrainer(DqnTrainerBase):
    def __init__(self, q_net: Optional[QNetwork] = None, lr: float = 1e-4, gamma: float = 0.98,
                 target_update_interval: int = 10_000, max_grad_norm: float = 10.0, double_q: bool = False,
                 device: str = "cpu", force_collective: bool = False):
        super().__init__(target_update_interval, force_collective)
        self.q_net = (q_net if q_net is not None else QNetwork()).to(device)
        self._params = [p for p in self.q_net.parameters()]
        self._bucket = torch.zeros(sum(p.numel() for p in self._params), dtype=torch.float32, device=device)
        if self.world > 1:
            # Replicas must START equal: the same averaged gradient applied to different weights never re-converges.
            # Rank 0's weights win (whatever seeding or checkpoint loading happened before on the other ranks).
            with torch.no_grad():
                self._pack([p.detach() for p in self._params])
                dist.broadcast(self._bucket, src=0)
                self._unpack([p for p in self._params])
        self.q_net_target = copy.deepcopy(self.q_net).requires_grad_(False)
        self.optimizer = torch.optim.Adam(self.q_net.parameters(), lr=lr)
        self.gamma, self.max_grad_norm, self.double_q = gamma, max_grad_norm, double_q

    def td_target(self, rewards, next_obs, dones) -> torch.Tensor:
        with torch.no_grad():
            next_q = self.q_net_target(next_obs)
            if self.double_q:      # action chosen by the online net, valued by the target net
                best = self.q_net(next_obs).argmax(dim=1, keepdim=True)
                next_v = next_q.gather(1, best).squeeze(1)
            else:                  # vanilla DQN (the reference)
                next_v = next_q.max(dim=1).values
            return rewards + (1.0 - dones) * self.gamma * next_v

    def _pack(self, tensors):
        off = 0
        for t in tensors:
            n = t.numel()
            self._bucket[off:off + n].copy_(t.reshape(-1))
            off += n

    def _unpack(self, tensors, scale: Optional[float] = None):
        off = 0
        for t in tensors:
            n = t.numel()
            src = self._bucket[off:off + n].view_as(t)
            t.copy_(src if scale is None else src * scale)
            off += n

    def _all_reduce_gradients(self):
        """One flat bucket: pack, sum over ranks, average, unpack."""
        self._pack([p.grad for p in self._params])
        dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM)
        self._unpack([p.grad for p in self._params], 1.0 / self.world)

    def assert_replicas_equal(self) -> None:
        """Debug aid: every rank holds bit-identical online weights (max - min over ranks of the flat bucket is 0)."""
        if self.world == 1:
            return
        with torch.no_grad():
            self._pack([p.detach() for p in self._params])
            hi, lo = self._bucket.clone(), self._bucket.clone()
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            if not torch.equal(hi, lo):
                raise AssertionError(f"Q-network replicas differ across ranks (max |diff| {float((hi - lo).abs().max()):.3e})")

    def update(self, batch: Dict[str, torch.Tensor]) -> float:
        """batch (this rank's shard): obs [b,46] f32, actions [b] i64, rewards [b], next_obs [b,46], dones [b]; with
        ``weights`` [b] f32 (prioritized replay) the loss is weighted per row and ``last_td_error`` [b] holds the TD errors."""
        loss = self._eager_step(batch)
        self._count_updates()
        return loss

    # ---- hipGraph path: the update is ~40 tiny kernels (MLP forward / backward, Huber loss, clip, Adam) on 1 177
    # parameters, i.e. pure launch latency; captured once, it replays as ONE graph launch
    def enable_graph(self, batch_size: int, obs_dim: int = 46, weighted: bool = False) -> None:
        """Capture ``update`` for a fixed batch size into HIP graphs (``torch.cuda.CUDAGraph`` is hipGraph on ROCm).
        One process: ONE graph.  Several ranks: TWO graphs with the flat-bucket all-reduce between them -- graph A =
        forward, backward and packing the gradients into the bucket; the collective (RCCL) is enqueued eagerly on the same
        stream; graph B = averaging, unpacking, clipping and the Adam step.  Every rank must call this (the warm-up steps
        contain collectives).  ``weighted``: the captured update takes a static ``weights`` input and leaves the TD errors
        in the static tensor ``last_td_error`` (prioritized replay)."""
        dev = self._bucket.device
        if dev.type != "cuda":
            raise RuntimeError("enable_graph needs the GPU")
        lr = self.optimizer.param_groups[0]["lr"]
        self.optimizer = torch.optim.Adam(self.q_net.parameters(), lr=lr, capturable=True)
        self._g_batch = dict(obs=torch.zeros(batch_size, obs_dim, device=dev), actions=torch.zeros(batch_size, dtype=torch.int64, device=dev),
                             rewards=torch.zeros(batch_size, device=dev), next_obs=torch.zeros(batch_size, obs_dim, device=dev),
                             dones=torch.zeros(batch_size, device=dev))
        if weighted:
            self._g_batch["weights"] = torch.ones(batch_size, device=dev)
        self._g_loss = torch.zeros((), device=dev)
        before = [p.detach().clone() for p in self._params]     # _eager_step neither counts updates nor syncs the target
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up off the capture (allocations, Adam state)
            for _ in range(3):
                self._eager_step(self._g_batch)
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        if not self._collective:
            with torch.cuda.graph(self._graph):
                self._g_loss.copy_(self._eager_step(self._g_batch))
        else:
            with torch.cuda.graph(self._graph):
                self._g_loss.copy_(self._backward(self._g_batch))
                self._pack([p.grad for p in self._params])
            self._graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph_b, pool=self._graph.pool()):
                self._unpack([p.grad for p in self._params], 1.0 / self.world)
                self._apply()
        with torch.no_grad():                              # undo the warm-up / capture steps on the zero batch
            for p, p0 in zip(self._params, before):
                p.copy_(p0)
            for st in self.optimizer.state.values():
                st["exp_avg"].zero_(); st["exp_avg_sq"].zero_(); st["step"].zero_()

    def _backward(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        target = self.td_target(batch["rewards"], batch["next_obs"], batch["dones"])
        q = self.q_net(batch["obs"]).gather(1, batch["actions"].view(-1, 1)).squeeze(1)
        if "weights" in batch:
            # prioritized replay: mean(w_i * huber(delta_i)), every row weighted by ITS importance weight, and the TD errors
            # delta = target - Q(s, a) kept on the device for the re-prioritization (deviation 3)
            self.last_td_error = (target - q).detach()
            loss = (batch["weights"] * F.smooth_l1_loss(q, target, reduction="none")).mean()
        else:
            loss = F.smooth_l1_loss(q, target)
        self.optimizer.zero_grad(set_to_none=False)
        loss.backward()
        return loss.detach()

    def _apply(self) -> None:
        nn.utils.clip_grad_norm_(self._params, self.max_grad_norm)
        self.optimizer.step()

    def _eager_step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        loss = self._backward(batch)
        if self._collective:
            self._all_reduce_gradients()
        self._apply()
        return loss

    def update_graphed(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Same arithmetic as :meth:`update`, replayed from the captured graph(s) (batch size fixed by enable_graph)."""
        for k, v in self._g_batch.items():
            v.copy_(batch[k])
        self._graph.replay()
        if self._collective:
            dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM)
            self._graph_b.replay()
        self._count_updates()
        return self._g_loss

    def load_optimizer_state(self, sd: Dict) -> None:
        """Restore Adam's moments and step counts.  Once ``enable_graph`` has captured the update, the graph is bound to the
        optimiser's state TENSORS: ``Optimizer.load_state_dict`` would replace them with new ones that the replayed graph never
        sees (the restored moments would be ignored and later checkpoints would save the stale copies), so the loaded values
        are copied IN PLACE into the tensors the graph updates."""
        if not hasattr(self, "_graph"):
            self.optimizer.load_state_dict(sd)
            return
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        if len(ids) != len(params):
            raise ValueError(f"optimizer checkpoint holds {len(ids)} parameters, this optimizer {len(params)}")
        # everything the captured graph has baked in is compared BEFORE anything is copied: a checkpoint that does not fit must
        # leave the live optimiser state as it was
        if len(sd["param_groups"]) != len(self.optimizer.param_groups):
            raise ValueError(f"optimizer checkpoint holds {len(sd['param_groups'])} parameter groups, this optimizer {len(self.optimizer.param_groups)}")
        for g, gs in zip(self.optimizer.param_groups, sd["param_groups"]):
            for key in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
                as_tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,)
                if key in g and key in gs and as_tuple(g[key]) != as_tuple(gs[key]):
                    raise ValueError(f"the captured graph holds the optimiser's {key} = {g[key]!r} it was captured with; the checkpoint has "
                                     f"{gs[key]!r} (load it before enable_graph, or capture again)")
        for p, i in zip(params, ids):
            src = sd["state"].get(i)
            if src is not None:
                for k in ("exp_avg", "exp_avg_sq"):
                    if tuple(torch.as_tensor(src[k]).shape) != tuple(self.optimizer.state[p][k].shape):
                        raise ValueError(f"optimizer checkpoint: {k} of parameter {i} has shape {tuple(torch.as_tensor(src[k]).shape)}, "
                                         f"expected {tuple(self.optimizer.state[p][k].shape)}")
        with torch.no_grad():
            for p, i in zip(params, ids):
                st, src = self.optimizer.state[p], sd["state"].get(i)
                for k in ("exp_avg", "exp_avg_sq", "step"):
                    if src is None:
                        st[k].zero_()
                    else:
                        st[k].copy_(torch.as_tensor(src[k]).to(device=st[k].device, dtype=st[k].dtype))

    def theta(self) -> torch.Tensor:
        return torch.cat([p.detach().reshape(-1) for p in self._params]).to(dtype=torch.float32).contiguous()

    def sync_target(self) -> None:
        """Hard target update (SB3 ``polyak_update`` with tau = 1)."""
        self.q_net_target.load_state_dict(self.q_net.state_dict())
        self.num_target_syncs += 1


# ----------------------------------------------------------------------------------------------------------------------
# collection + learning loop over the batched environment (SB3 ``DQN.learn`` semantics of the reference's training
# script: src/test_block_rl.py:68-86 -- n_envs vectorised environments, learning_starts 50 000, train_freq 4 steps,
# gradient_steps -1 (one gradient step per collected transition), batch 32, buffer 1e6, epsilon 1.0 -> 0.05 over the
# first 20 % of the run, hard target update every 10 000 environment steps)
# ----------------------------------------------------------------------------------------------------------------------
def flatten_observation(obs: Dict[str, torch.Tensor]) -> torch.Tensor:
    """SB3's CombinedExtractor concatenates the dict entries in sorted key order: ``external`` (32) then ``internal``
    (14) -- the input layout of the reference's trained network (see dqn.py)."""
    return torch.cat([obs["external"], obs["internal"]], dim=1)


class ReplayBuffer:
    """``ReplayBuffer(capacity, obs_dim, device)``: ring buffer, resident on the environment's device (transitions never visit
    the host), written against ``FIELDS`` and three hooks for the observation storage (:class:`ImageReplayBuffer`).  Uniform
    (``sum_tree`` is None) unless ``per_kwargs``, a dictionary, makes it prioritized experience replay: the priorities of the
    stored transitions are the leaves of a device-resident sum tree (:class:`per_tree.SumTree`, csrc/pergpu.hip).  Keyword names
    are the reference's (``PerReplayBuffer``, src/pkg_dqn/utils/per_dqn.py:43-56); ``refresh_tree_freq`` is accepted and
    ignored -- inner nodes here are always the sum of their children and never drift."""

    FIELDS = ("obs", "next_obs", "actions", "rewards", "dones")

    def __init__(self, capacity: int, *shape_and_device, per_kwargs: Optional[Dict] = None):
        *shape, self.device = shape_and_device
        self.capacity = int(capacity)
        self._allocate_obs(*shape)
        self.actions = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self.rewards = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
        self.dones = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
        self.pos, self.size = 0, 0
        self.sum_tree = None if per_kwargs is None else SumTree(
            self.capacity, self.device, **{k: v for k, v in per_kwargs.items() if k != "refresh_tree_freq"})

    def _allocate_obs(self, obs_dim: int) -> None:
        self.obs = torch.zeros(self.capacity, obs_dim, dtype=torch.float32, device=self.device)
        self.next_obs = torch.zeros_like(self.obs)

    def _store_obs(self, idx: torch.Tensor, obs, next_obs) -> None:
        self.obs[idx], self.next_obs[idx] = obs, next_obs

    def _read_obs(self, idx: torch.Tensor, prefix: str):       # prefix "": the observations of the rows idx; "next_": the next ones
        return getattr(self, prefix + "obs")[idx]

    def add(self, obs, next_obs, actions, rewards, dones) -> None:
        n = actions.shape[0]
        if self.sum_tree is not None:
            self.sum_tree.add(self.pos, n, self.size)      # the new rows take the running maximum priority
        idx = (self.pos + torch.arange(n, device=self.device)) % self.capacity
        self._store_obs(idx, obs, next_obs)
        self.actions[idx] = actions.to(torch.int64)
        self.rewards[idx] = rewards.to(torch.float32)
        self.dones[idx] = dones.to(torch.float32)
        self.pos, self.size = (self.pos + n) % self.capacity, min(self.size + n, self.capacity)

    def sample(self, n: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """Uniform; with the sum tree stratified by priority, and the batch then also holds ``indices`` (tree indices, for
        :meth:`update_priorities`) and ``weights`` (importance weights, float32, normalised by their maximum)."""
        if self.sum_tree is None:
            return self._rows(torch.randint(0, self.size, (n,), device=self.device, generator=generator))
        u = torch.rand(n, dtype=torch.float64, device=self.device, generator=generator)
        indices, positions, weights = self.sum_tree.sample(u, self.size)
        return dict(self._rows(positions), indices=indices, weights=weights)

    def _rows(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        return dict(obs=self._read_obs(idx, ""), actions=self.actions[idx], rewards=self.rewards[idx],
                    next_obs=self._read_obs(idx, "next_"), dones=self.dones[idx])

    def update_priorities(self, indices: torch.Tensor, td_error: torch.Tensor) -> None:
        self.sum_tree.update(indices, td_error)

    def state_dict(self) -> Dict:
        n = self.size
        return dict(pos=self.pos, size=n, **{k: getattr(self, k)[:n].clone() for k in self.FIELDS},
                    **({} if self.sum_tree is None else dict(per=self.sum_tree.state_dict(n))))

    def load_state_dict(self, src: Dict) -> None:
        n = src["size"]
        if n > self.capacity:
            raise ValueError(f"checkpointed buffer holds {n} transitions, this buffer only {self.capacity}")
        for k in self.FIELDS:
            getattr(self, k)[:n] = src[k].to(self.device)
        self.pos, self.size = src["pos"] % self.capacity, n
        if self.sum_tree is not None:
            self.sum_tree.load_state_dict(src["per"])


class ImageReplayBuffer(ReplayBuffer):
    """The same ring buffer for the image observation, ``ImageReplayBuffer(capacity, image_shape, n_internal, device)``:
    images stay uint8 (3 H W bytes each, 8 748 at 54 x 54), the internal observation float32.  One transition holds two
    observations: 17.6 KB at 54 x 54, so the reference's default of 1e6 transitions takes 17.6 GB of device memory."""

    FIELDS = ("img", "next_img", "internal", "next_internal", "actions", "rewards", "dones")

    def _allocate_obs(self, image_shape, n_internal: int) -> None:
        self.img = torch.zeros((self.capacity,) + tuple(image_shape), dtype=torch.uint8, device=self.device)
        self.next_img = torch.zeros_like(self.img)
        self.internal = torch.zeros(self.capacity, n_internal, dtype=torch.float32, device=self.device)
        self.next_internal = torch.zeros_like(self.internal)

    def _store_obs(self, idx: torch.Tensor, obs, next_obs) -> None:
        self.img[idx], self.next_img[idx] = obs["external"], next_obs["external"]
        self.internal[idx], self.next_internal[idx] = obs["internal"], next_obs["internal"]

    def _read_obs(self, idx: torch.Tensor, prefix: str):
        return {"external": getattr(self, prefix + "img")[idx], "internal": getattr(self, prefix + "internal")[idx]}


def check_ray_buffer(buffer, device) -> None:
    """What every kernel that walks the replay ring itself assumes of ``buffer`` (``FusedDqnTrainer.train`` and ``train_per``,
    ``collect.collect_rays``): every field ``capacity`` rows of its dtype, contiguous and on ``device``, flat ray observations,
    and a sum tree, where there is one, of the buffer's capacity.  ``ValueError`` otherwise, before anything is enqueued."""
    C = buffer.capacity
    for name, dtype in (("obs", torch.float32), ("next_obs", torch.float32), ("actions", torch.int64),
                        ("rewards", torch.float32), ("dones", torch.float32)):
        x = getattr(buffer, name, None)
        if x is None or x.dtype != dtype or not x.is_contiguous() or x.device != device or x.shape[0] != C:
            raise ValueError(f"buffer.{name} must be {C} rows of contiguous {dtype} on {device}")
    if buffer.obs.shape[1:] != (OBS_DIM,) or buffer.next_obs.shape != buffer.obs.shape:
        raise ValueError(f"the buffer holds observations of shape {tuple(buffer.obs.shape[1:])}, not ({OBS_DIM},)")
    tree = getattr(buffer, "sum_tree", None)
    if tree is not None:
        t = tree.tree
        if tree.capacity != C or t.dtype != torch.float64 or not t.is_contiguous() or t.device != device or t.numel() != 2 * C - 1:
            raise ValueError(f"the sum tree must be {2 * C - 1} contiguous float64 values on {device}: the buffer's capacity is {C}, "
                             f"the tree's {tree.capacity}")


def _map_obs(fn, obs):
    """``fn`` of an observation the loop stands at: a tensor (rays), a dictionary of tensors (images) or None (no loop yet)."""
    if obs is None:
        return None
    return {k: fn(v) for k, v in obs.items()} if isinstance(obs, dict) else fn(obs)


def exploration_rate(step: int, total: int, fraction: float = 0.2, initial: float = 1.0, final: float = 0.05) -> float:
    """SB3 ``get_linear_fn``: linear from ``initial`` to ``final`` over the first ``fraction`` of the run."""
    progress = step / float(total)
    if progress > fraction:
        return final
    return initial + progress * (final - initial) / fraction


def make_trainer(env, fused: bool = False, **kw) -> DqnTrainerBase:
    """The trainer :class:`DqnLearner` defaults to on ``env``: :class:`dqn.ImageQNetwork` on an image environment, the fused
    HIP update (:class:`dqn_fused.FusedDqnTrainer`) with ``fused``; ``kw`` are the trainer's arguments."""
    kw.setdefault("device", str(env.device))
    if fused:
        from .dqn_fused import FusedDqnTrainer
        return FusedDqnTrainer(**kw)
    return DqnTrainer(q_net=ImageQNetwork(env.image_shape) if getattr(env, "is_image_env", False) else None, **kw)


class DqnLearner:
    """Collect with an epsilon-greedy policy on a batched environment and update the Q-network.

    ``env`` needs ``B``, ``device``, ``reset()`` and ``step(actions, auto_reset=True)`` with the contract of
    :class:`rl_env.BatchedRaysEnv`.  On an image environment (``env.is_image_env``, :class:`rl_env.BatchedImgsEnv`) the
    Q-network is :class:`dqn.ImageQNetwork`, observations stay dictionaries and the buffer keeps the images as uint8
    (:class:`ImageReplayBuffer`); its update runs eagerly (``use_graph`` is refused).  With ``torch.distributed`` initialised every rank drives its own shard of
    environments and its own buffer; gradients are summed by :class:`DqnTrainer`'s single flat all-reduce."""

    def __init__(self, env, trainer: Optional[DqnTrainer] = None, buffer_size: int = 1_000_000,
                 learning_starts: int = 50_000, batch_size: int = 32, train_freq: int = 4, gradient_steps: int = -1,
                 target_update_interval: int = 10_000, exploration_fraction: float = 0.2,
                 exploration_initial_eps: float = 1.0, exploration_final_eps: float = 0.05, seed: int = 0,
                 use_graph: bool = False, track_episodes: bool = True, per: bool = False,
                 per_kwargs: Optional[Dict] = None, fused: bool = False, per_in_kernel: bool = False,
                 collect_in_kernel: bool = False, collect_launch_steps: Optional[int] = None, collect_turnover: bool = False):
        """``per=True``: prioritized experience replay (the reference's ``'per': True``): the buffer keeps a sum tree of
        priorities (``per_kwargs``: alpha, beta, epsilon, update_max_freq, initial_priority), minibatches are drawn by
        priority, the loss is weighted by the importance weights and the drawn rows are re-prioritized with their TD errors
        after every update -- all on the device.  With several ranks every rank has its own tree.

        ``fused=True`` (ray environment only): the update is the fused HIP kernel of :class:`dqn_fused.FusedDqnTrainer`
        (DESIGN.md 8.6).  With uniform replay and one rank the whole update round of ``learn`` is ONE launch that draws its
        own minibatches from the counter stream ``(seed + rank, serial)`` -- both are part of ``state_dict`` --; with
        ``per=True`` or several ranks it is one fused update per step around the tree's kernels or the all-reduce.

        ``per_in_kernel=True`` (needs ``fused=True`` and ``per=True``, one rank): the round is ONE launch with prioritized
        replay too -- the kernel samples the tree, updates and re-prioritises step after step
        (:meth:`dqn_fused.FusedDqnTrainer.train_per`), its uniforms from the same counter stream.  The
        checkpoint has the same keys either way and moves between the two settings.

        ``collect_in_kernel=True`` (ray environment on one record table, any ray trainer): the ``train_freq`` steps a round of
        ``learn`` collects -- act, auto-reset step, buffer rows, episode returns -- are ONE launch of the step kernel
        (:func:`collect.collect_rays`), or launches of ``collect_launch_steps`` steps each (at most 64; the
        default is the whole round, under ``collect_turnover`` ``collect_fresh.DEFAULT_LAUNCH_STEPS``).  Exploration then draws from the counter stream ``(collect_seed, collect_serial)``, both
        part of ``state_dict``, instead of the torch generator, so the actions are not those of the host-driven loop; the
        target network is synchronised once behind a round whose steps reach the interval.

        ``collect_turnover=True`` (needs ``collect_in_kernel=True`` and a ray environment after ``enable_spares()`` /
        ``enable_fresh_maps()``): the launches are those of :func:`collect_fresh.collect_rays_fresh` on the two-record table
         -- a new map per episode without leaving the launch.  A refill of the spares stands behind a launch, never
        inside it: the run equals the one in launches of one step only where every refill point falls on the end of a launch
        (``refill_every`` a multiple of ``collect_launch_steps``, rounds that are whole launches)."""
        if collect_turnover and not collect_in_kernel:
            raise ValueError("collect_turnover=True needs collect_in_kernel=True: it is collection inside the launch on the "
                             "two-record table")
        if per_in_kernel and not (fused and per):
            raise ValueError("per_in_kernel=True needs fused=True and per=True: it is the prioritized form of the fused K-step launch")
        self.env, self.device = env, env.device
        self.image = bool(getattr(env, "is_image_env", False))
        if self.image and use_graph:
            raise ValueError("use_graph=True is not built for the image environment: its updates run eagerly")
        self.fused = bool(fused)
        if self.fused and self.image:
            raise ValueError("fused=True is built for the ray Q-network only: the image environment's updates run eagerly")
        if self.fused and use_graph:
            raise ValueError("fused=True and use_graph=True exclude each other: the fused update is one launch already")
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        if trainer is None:
            trainer = make_trainer(env, fused=self.fused)
        if self.fused:
            from .dqn_fused import FusedDqnTrainer
            if not isinstance(trainer, FusedDqnTrainer):
                raise ValueError("fused=True needs a dqn_fused.FusedDqnTrainer")
            trainer.seed, trainer.serial = seed + rank, 0
        self.trainer = trainer
        self.trainer.target_update_interval = 0   # the learner syncs on environment steps, as SB3 does
        self.per = bool(per)
        self.buffer = (ImageReplayBuffer if self.image else ReplayBuffer)(
            buffer_size, *((env.image_shape, 14) if self.image else (46,)), self.device,
            per_kwargs=(per_kwargs or {}) if self.per else None)
        self.learning_starts, self.batch_size, self.train_freq = learning_starts, batch_size, train_freq
        self.gradient_steps, self.target_update_interval = gradient_steps, target_update_interval
        self.eps = (exploration_fraction, exploration_initial_eps, exploration_final_eps)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + rank)
        self.num_timesteps, self.n_calls = 0, 0
        self.episode_returns, self.episode_successes = [], []
        # track_episodes=False keeps the episode statistics as device counters (no host synchronisation in the loop)
        self.track_episodes = track_episodes
        self.ep_count, self.ep_return_sum, self.ep_success_sum = (torch.zeros((), dtype=torch.float64, device=self.device) for _ in range(3))
        if use_graph:
            self.trainer.enable_graph(batch_size, weighted=self.per)
        # decided once: one step's update, whether a round is ONE launch that samples the buffer itself (fused, one rank, uniform
        # or per_in_kernel), and with that the round's update; the round's collection at the end of the constructor
        self._update = self.trainer.update_graphed if use_graph else self.trainer.update
        self.per_in_kernel = bool(per_in_kernel)
        if self.per_in_kernel and self.trainer.collective:
            raise ValueError("per_in_kernel=True is the one-rank path: several ranks (or force_collective) update step by step "
                             "around the all-reduce")
        self._one_launch = self.fused and (not self.per or self.per_in_kernel) and not self.trainer.collective
        self._train = self.trainer.train_per if self.per_in_kernel else getattr(self.trainer, "train", None)
        self._update_round = self._update_in_one_launch if self._one_launch else self._update_step_by_step
        # state of the collection loop between two learn() calls (a run can be checkpointed and resumed in the middle)
        self._obs, self._ep_return, self.n_updates = None, None, 0
        self._last_loss = torch.zeros((), device=self.device)
        self.collect_in_kernel, self.collect_turnover = bool(collect_in_kernel), bool(collect_turnover)
        if self.collect_in_kernel:
            from . import collect, collect_fresh, dqn_fused
            (collect_fresh if self.collect_turnover else collect).check_env(env)
            self._collect_launch = collect_fresh.collect_rays_fresh if self.collect_turnover else collect.collect_rays
            dqn_fused.check_shape(self.trainer.q_net)
            if collect_launch_steps is not None and int(collect_launch_steps) < 1:
                raise ValueError("collect_launch_steps must be at least 1")
            default = collect_fresh.DEFAULT_LAUNCH_STEPS if self.collect_turnover else collect.MAX_STEPS
            self.collect_launch_steps = default if collect_launch_steps is None else min(int(collect_launch_steps), collect.MAX_STEPS)
            # not the trainer's fused_seed (seed + rank): minibatch rows and exploration must not share a stream
            self.collect_seed, self.collect_serial = ((seed + rank) ^ 0x436F6C6C65637421) % 2 ** 64, 0
            self._collect_out = None
        self._collect = self._collect_in_kernel if self.collect_in_kernel else self._collect_on_host

    def _prepare(self, obs):
        """The network's input: the flat vector for rays, the dictionary itself for images."""
        return obs if self.image else flatten_observation(obs)

    def act(self, obs_flat: torch.Tensor, epsilon: float) -> torch.Tensor:
        greedy = self.trainer.q_net.greedy_actions(obs_flat)
        B = greedy.shape[0]
        explore = torch.rand(B, device=self.device, generator=self.gen) < epsilon
        rand = torch.randint(0, 9, (B,), device=self.device, generator=self.gen)
        return torch.where(explore, rand, greedy)

    # ---- checkpoint / resume: what SB3's model.save / EvalCallback(best_model_save_path) / Algorithm.load do for the
    # reference (src/test_block_rl.py:73-76,89-96), extended by everything an EXACT continuation needs -- optimiser moments,
    # counters, random generator, replay buffer, the environments' own state and the observation the loop stands at.
    def state_dict(self, include_buffer: bool = True) -> Dict:
        tr = self.trainer
        d = dict(q_net=tr.q_net.state_dict(), q_net_target=tr.q_net_target.state_dict(), optimizer=tr.optimizer.state_dict(),
                 num_updates=tr.num_updates, num_target_syncs=tr.num_target_syncs,
                 num_timesteps=self.num_timesteps, n_calls=self.n_calls, n_updates=self.n_updates,
                 generator=self.gen.get_state(), episode_returns=list(self.episode_returns),
                 episode_successes=list(self.episode_successes), ep_count=self.ep_count.clone(),
                 ep_return_sum=self.ep_return_sum.clone(), ep_success_sum=self.ep_success_sum.clone(),
                 obs=_map_obs(torch.clone, self._obs), ep_return=_map_obs(torch.clone, self._ep_return))
        if self.fused:
            d["fused_seed"], d["fused_serial"] = tr.seed, tr.serial
        if self.collect_in_kernel:
            d["collect_seed"], d["collect_serial"] = self.collect_seed, self.collect_serial
            if self._obs is not None:     # the loop stands at the observation the environment holds
                d["obs"] = self._prepare(self.env._obs())
        if include_buffer:
            d["buffer"] = self.buffer.state_dict()
        if hasattr(self.env, "state_dict"):
            d["env"] = self.env.state_dict()
        return d

    def load_state_dict(self, d: Dict) -> None:
        tr = self.trainer
        tr.q_net.load_state_dict(d["q_net"]); tr.q_net_target.load_state_dict(d["q_net_target"])
        tr.load_optimizer_state(d["optimizer"])     # in place when the update has been captured into a graph
        tr.num_updates, tr.num_target_syncs = d["num_updates"], d["num_target_syncs"]
        if self.fused:
            tr.seed, tr.serial = d["fused_seed"], d["fused_serial"]
        if self.collect_in_kernel and "collect_seed" in d:
            self.collect_seed, self.collect_serial = d["collect_seed"], d["collect_serial"]
        self.num_timesteps, self.n_calls, self.n_updates = d["num_timesteps"], d["n_calls"], d["n_updates"]
        self.gen.set_state(d["generator"].cpu())   # a generator state is a host ByteTensor, also for a device generator
        self.episode_returns, self.episode_successes = list(d["episode_returns"]), list(d["episode_successes"])
        self.ep_count.copy_(d["ep_count"]); self.ep_return_sum.copy_(d["ep_return_sum"]); self.ep_success_sum.copy_(d["ep_success_sum"])
        self._obs, self._ep_return = (_map_obs(lambda v: v.to(self.device), d[k]) for k in ("obs", "ep_return"))
        if "buffer" in d:
            self.buffer.load_state_dict(d["buffer"])
        if "env" in d and hasattr(self.env, "load_state_dict"):
            self.env.load_state_dict(d["env"])

    def save(self, path: str, include_buffer: bool = True) -> None:
        torch.save(self.state_dict(include_buffer), path)

    def load(self, path: str) -> None:
        # tensors, numbers, lists and dicts only (the generator state is a ByteTensor): no pickled code is executed
        self.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))

    def save_model(self, path: str) -> None:
        """The policy alone (the reference's final_model / best_model): the Q-network's weights."""
        torch.save(self.trainer.q_net.state_dict(), path)

    def _account_episodes(self, done: torch.Tensor, success: torch.Tensor, episode_return: torch.Tensor) -> None:
        """The episodes that ended in ``done`` ([B] of one step or [T, B] of one launch: t, then b ascending) into the tracked
        lists or the two device counts, which are sums of integers and exact in float64 in any order.  ``ep_return_sum`` is each
        round's own: its per-step sums are formed from different tensors and keep their bits only as they stand."""
        if self.track_episodes:
            if bool(done.any()):
                self.episode_returns += episode_return[done].tolist()
                self.episode_successes += success[done].tolist()
        else:
            self.ep_count += done.sum()
            self.ep_success_sum += (success & done).sum()

    def _sync_due(self, since: int, until: int) -> bool:
        """Whether one of the environment calls ``since + 1 .. until`` reaches ``target_update_interval`` (in calls of B steps)."""
        every = max(self.target_update_interval // self.env.B, 1)
        return any(call % every == 0 for call in range(since + 1, until + 1))

    # ---- the two collection rounds, one of them bound as ``_collect`` in __init__: up to ``train_freq`` calls of the environment with
    # the schedule's epsilons, buffer rows, episode statistics, counters and the target sync.  Both return the transitions collected.
    def _collect_on_host(self, total_timesteps: int) -> int:
        """One round driven from the host: act, auto-reset step and ``buffer.add`` per call, the sync at the call that is due one."""
        env, B, collected = self.env, self.env.B, 0
        obs, ep_return = self._obs, self._ep_return
        for _ in range(self.train_freq):
            eps = exploration_rate(self.num_timesteps, total_timesteps, *self.eps)
            actions = self.act(obs, eps)
            nxt, reward, terminated, truncated, info = env.step(actions, auto_reset=True)
            done = terminated | truncated
            nxt_flat = self._prepare(nxt)
            # the transition stores the observation the episode ended in, not the first one of the next episode;
            # a time-limit truncation is not a terminal state for the bootstrap (SB3 handle_timeout_termination)
            stored_next = self._prepare(info["terminal_observation"]) if "terminal_observation" in info else nxt_flat
            self.buffer.add(obs, stored_next, actions, reward, terminated)
            ep_return += reward
            self._account_episodes(done, info["success"], ep_return)
            if not self.track_episodes:
                self.ep_return_sum += (ep_return * done).sum()
            ep_return = torch.where(done, torch.zeros_like(ep_return), ep_return)
            obs = nxt_flat
            self.num_timesteps += B
            self.n_calls += 1
            collected += B
            if self._sync_due(self.n_calls - 1, self.n_calls):
                self.trainer.sync_target()
            if self.num_timesteps >= total_timesteps:
                break
        self._obs, self._ep_return = obs, ep_return
        return collected

    def _collect_in_kernel(self, total_timesteps: int) -> int:
        """One round inside the step kernel (``collect_in_kernel``): the steps the host-driven round would make, with its
        epsilons, in launches of ``collect_launch_steps``; the episode statistics from the [T, B] outputs, and ONE target sync
        behind the round if any of its steps is due one."""
        from . import collect
        B, ep_return = self.env.B, self._ep_return
        n = min(self.train_freq, -(-(total_timesteps - self.num_timesteps) // B))
        theta = self.trainer.theta()
        if self._collect_out is None:
            self._collect_out = {name: torch.zeros(self.collect_launch_steps, B, dtype=dtype, device=self.device)
                                 for name, dtype in collect.OUTPUTS}
        sync, made = False, 0
        while made < n:
            T = min(n - made, self.collect_launch_steps)
            eps = [exploration_rate(self.num_timesteps + t * B, total_timesteps, *self.eps) for t in range(T)]
            out = {name: x[:T] for name, x in self._collect_out.items()}
            self._collect_launch(self.env, theta, self.buffer, eps, self.collect_seed, self.collect_serial, ep_return, out)
            done, ended = out["done"].bool(), out["episode_return"]
            self._account_episodes(done, out["success"].bool(), ended)
            if not self.track_episodes:       # per step, as the host-driven round sums: the same bits whatever the launch size
                for t in range(T):
                    self.ep_return_sum += torch.where(done[t], ended[t], torch.zeros_like(ep_return)).sum()
            sync = sync or self._sync_due(self.n_calls, self.n_calls + T)
            self.collect_serial += T
            self.num_timesteps += T * B
            self.n_calls += T
            made += T
        if sync:
            self.trainer.sync_target()
        return n * B

    # ---- the two update rounds, one of them bound as ``_update_round`` in __init__: ``steps`` >= 1 gradient steps -> the last loss
    def _update_in_one_launch(self, steps: int) -> torch.Tensor:
        """The round as ONE launch that draws its minibatches itself (``train``, or ``train_per`` with ``per_in_kernel``)."""
        return self._train(self.buffer, steps, self.batch_size)[-1]

    def _update_step_by_step(self, steps: int) -> torch.Tensor:
        """Sample, update (eager, a replayed graph or the fused kernel: ``_update``), re-prioritize, ``steps`` times."""
        for _ in range(steps):
            batch = self.buffer.sample(self.batch_size, self.gen)
            loss = self._update(batch)
            if self.per:      # the PER kernels run eagerly on the same stream, around the (possibly replayed) update
                self.buffer.update_priorities(batch["indices"], self.trainer.last_td_error)
        return loss

    def learn(self, total_timesteps: int, callback: Optional[Callable[["DqnLearner"], None]] = None,
              stop_at: Optional[int] = None) -> Dict[str, float]:
        """Collect and learn until ``total_timesteps`` (the horizon of the exploration schedule) -- or until ``stop_at``, a
        point to checkpoint at; a later call, also on a learner restored with ``load``, continues exactly there."""
        if self._obs is None:
            self._obs = self._prepare(self.env.reset())
            self._ep_return = torch.zeros(self.env.B, dtype=torch.float64, device=self.device)
        end = total_timesteps if stop_at is None else min(stop_at, total_timesteps)
        while self.num_timesteps < end:
            collected = self._collect(total_timesteps)
            if self.num_timesteps > self.learning_starts and self.buffer.size >= self.batch_size:
                steps = self.gradient_steps if self.gradient_steps >= 0 else collected
                if steps > 0:
                    self._last_loss = self._update_round(steps)
                self.n_updates += steps
            if callback is not None:
                callback(self)
        stats = dict(timesteps=self.num_timesteps, updates=self.n_updates, loss=float(self._last_loss))
        if not self.track_episodes:       # whole-run averages from the device counters
            n = float(self.ep_count)
            return dict(stats, episodes=int(n), mean_return=float(self.ep_return_sum) / n if n else float("nan"),
                        success_rate=float(self.ep_success_sum) / n if n else float("nan"))
        recent = self.episode_returns[-100:]
        return dict(stats, episodes=len(self.episode_returns), mean_return=float(sum(recent) / len(recent)) if recent else float("nan"),
                    success_rate=float(sum(self.episode_successes[-100:]) / max(1, len(self.episode_successes[-100:]))))
