"""Batched visibility-graph shortest paths: host side of ``include/mpcgpu_plan.h``.

The reference plans a reference path on every reset with ``extremitypathfinder`` on mitred outlines
(``src/pkg_dqn/environment/environment.py:122-146,165-168``).  Here one launch of ``csrc/plangpu.hip`` plans a whole batch
of maps; this module orients and packs the rings, applies the reference's inflation (``rl_geometry.mitre_polygon``) and
hands the paths back.  There is no fallback: without the built library and a HIP device, planning raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import rl_geometry as rg
from .solver import MpcGpuError, bind_exports, load_library

MAX_VERTICES = 256
MAX_RINGS = 32
MAX_PATH_NODES = 64
STATUS = {0: "ok", 1: "no path", 2: "start or goal not in free space", 3: "more than 64 path nodes", 4: "malformed record"}


class _CPlanParams(C.Structure):
    _fields_ = [("n_vert_max", C.c_int32), ("n_ring_max", C.c_int32), ("n_node_max", C.c_int32), ("reserved", C.c_int32)]


_VP, _I32, _PP = C.c_void_p, C.c_int32, C.POINTER(_CPlanParams)
# export -> (restype, argtypes); include/mpcgpu_plan.h
_PLAN_TABLE = {
    "mpcgpu_plan_record_doubles": (_I32, [_PP]),
    "mpcgpu_plan_paths_dev": (_I32, [_I32, _PP, _I32] + [_VP] * 7),
    "mpcgpu_plan_last_error": (C.c_char_p, []),
}
PLAN_EXPORTS = tuple(_PLAN_TABLE)


def _bind(lib):
    return bind_exports(lib, "plan", _PLAN_TABLE, "csrc/plangpu.hip")


def oriented_rings(boundary, obstacles: Sequence) -> List[np.ndarray]:
    """[boundary counter-clockwise, obstacles clockwise]: open float64 rings, the order the kernel and its twin expect."""
    return [rg.orient(boundary, ccw=True)] + [rg.orient(o, ccw=False) for o in obstacles]


def record_doubles(n_vert_max: int, n_ring_max: int) -> int:
    r = 2 + n_ring_max + 2 * n_vert_max
    return r + (r & 1)


def pack_rings(ring_lists: Sequence[Sequence[np.ndarray]], n_vert_max: Optional[int] = None,
               n_ring_max: Optional[int] = None) -> Tuple[np.ndarray, Dict]:
    """Oriented ring lists (one per map) -> (records [B, R] float64, dict(n_vert_max, n_ring_max)); layout:
    include/mpcgpu_plan.h.  The capacities default to the batch maxima; the library refuses more than 256 vertices or
    32 rings per map."""
    V = max([3] + [sum(len(r) for r in rings) for rings in ring_lists])
    R = max([1] + [len(rings) for rings in ring_lists])
    if n_vert_max is not None:
        if V > n_vert_max:
            raise ValueError(f"a map has {V} ring vertices, the table only {n_vert_max}")
        V = int(n_vert_max)
    if n_ring_max is not None:
        if R > n_ring_max:
            raise ValueError(f"a map has {R} rings, the table only {n_ring_max}")
        R = int(n_ring_max)
    rec = np.zeros((len(ring_lists), record_doubles(V, R)))
    for b, rings in enumerate(ring_lists):
        if any(len(r) < 3 for r in rings):
            raise ValueError("a ring needs at least three vertices")
        rec[b, 0], rec[b, 1] = len(rings), sum(len(r) for r in rings)
        rec[b, 2:2 + len(rings)] = [len(r) for r in rings]
        xy = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]).reshape(-1)
        rec[b, 2 + R:2 + R + len(xy)] = xy
    return rec, dict(n_vert_max=V, n_ring_max=R)


class PathPlanner:
    """Plans batches of maps on the GPU.  Rings are taken as they are (already inflated); orientation is normalised."""

    def __init__(self, device: int = 0, n_node_max: int = MAX_PATH_NODES):
        import torch
        if not torch.cuda.is_available():
            raise MpcGpuError("PathPlanner needs a HIP device: the planner is a GPU kernel, there is no CPU path")
        self._torch = torch
        self._lib = _bind(load_library())
        self.device = torch.device("cuda", device)
        self.device_index = device
        self.n_node_max = int(n_node_max)

    def plan_dev(self, records, start_goal, n_vert_max: int, n_ring_max: int, out=None):
        """Device tensors in, device tensors out, nothing synchronises: ``records`` [B, R] and ``start_goal`` [B, 4]
        float64 -> (status int32 [B], n_nodes int32 [B], nodes float64 [B, 64, 2], length float64 [B]).  ``out``: the
        four tensors of an earlier call, written again instead of allocating new ones."""
        torch = self._torch
        params = _CPlanParams(int(n_vert_max), int(n_ring_max), self.n_node_max, 0)
        R = self._lib.mpcgpu_plan_record_doubles(C.byref(params))
        if R < 0:
            raise MpcGpuError(self._lib.mpcgpu_plan_last_error().decode())
        B = records.shape[0]
        if records.shape != (B, R) or start_goal.shape != (B, 4) or records.dtype != torch.float64 or \
                start_goal.dtype != torch.float64 or not records.is_contiguous() or not start_goal.is_contiguous():
            raise ValueError(f"records must be contiguous float64 [B, {R}] and start_goal float64 [B, 4]")
        if out is not None:
            status, n_nodes, nodes, length = out
        else:
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            n_nodes = torch.empty(B, dtype=torch.int32, device=self.device)
            nodes = torch.empty(B, MAX_PATH_NODES, 2, dtype=torch.float64, device=self.device)
            length = torch.empty(B, dtype=torch.float64, device=self.device)
        rc = self._lib.mpcgpu_plan_paths_dev(self.device_index, C.byref(params), B, records.data_ptr(), start_goal.data_ptr(),
                                             status.data_ptr(), n_nodes.data_ptr(), nodes.data_ptr(), length.data_ptr(),
                                             torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise MpcGpuError(self._lib.mpcgpu_plan_last_error().decode())
        return status, n_nodes, nodes, length

    def plan(self, boundaries: Sequence, obstacle_lists: Sequence[Sequence], starts, goals):
        """One boundary ring, one list of obstacle rings, one start and one goal per map -> (status int32 [B], n_nodes
        int32 [B], length float64 [B], paths: list of float64 [n_nodes, 2], empty unless status 0)."""
        torch = self._torch
        ring_lists = [oriented_rings(b, o) for b, o in zip(boundaries, obstacle_lists)]
        rec, caps = pack_rings(ring_lists)
        sg = np.concatenate([np.asarray(starts, dtype=np.float64).reshape(len(ring_lists), -1)[:, :2],
                             np.asarray(goals, dtype=np.float64).reshape(len(ring_lists), -1)[:, :2]], axis=1)
        status, n_nodes, nodes, length = self.plan_dev(torch.from_numpy(rec).to(self.device),
                                                       torch.from_numpy(np.ascontiguousarray(sg)).to(self.device), **caps)
        status, n_nodes, nodes, length = (t.cpu().numpy() for t in (status, n_nodes, nodes, length))
        paths = [nodes[b, :n_nodes[b]].copy() if status[b] == 0 else np.zeros((0, 2)) for b in range(len(ring_lists))]
        return status, n_nodes, length, paths


def inflate_spec(spec: Dict, obstacle_margin: float = 0.8, boundary_margin: float = 0.5):
    """(boundary ring, obstacle rings) of a map spec as the reference's path planning sees them (environment.py:130-140):
    the static obstacles grown by ``obstacle_margin``, the boundary shrunk by ``boundary_margin``, mitred joins with limit
    2; dynamic obstacles are not visible on the reference path.  Coordinates pass through float32 first, as ``make_map``'s."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # noqa: E731
    boundary = rg.mitre_polygon(f32(rg.orient(spec["boundary"])), -boundary_margin)
    return boundary, [rg.mitre_polygon(f32(rg.orient(nodes)), obstacle_margin) for nodes in spec["static"]]


def plan_reference_paths(specs: Sequence[Dict], obstacle_margin: float = 0.8, boundary_margin: float = 0.5, device: int = 0,
                         planner: Optional[PathPlanner] = None):
    """Reference paths of map specs (``boundary``, ``static``, ``start``, ``goal`` as :func:`rl_env.make_map` takes them)
    -> (paths, status): ``paths[i]`` is float64 [n, 2] from start to goal, or ``None`` where ``status[i] != 0`` -- the
    caller draws another map then, as environment.py:165-168 does."""
    inflated = [inflate_spec(s, obstacle_margin, boundary_margin) for s in specs]
    planner = planner or PathPlanner(device)
    goals = [np.asarray(s["goal"], dtype=np.float32).astype(np.float64)[:2] for s in specs]
    status, _, _, paths = planner.plan([b for b, _ in inflated], [o for _, o in inflated],
                                       [np.asarray(s["start"], dtype=np.float64)[:2] for s in specs], goals)
    return [p if st == 0 else None for p, st in zip(paths, status)], status
