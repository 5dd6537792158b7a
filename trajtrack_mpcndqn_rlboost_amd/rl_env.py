"""Batched DRL environment: host side of ``mpcgpu_env_step_dev``.

Mirrors ``TrajectoryPlannerEnvironmentRaysReward1`` of the reference (``src/pkg_dqn/environment/variants/
rays_reward1.py:7-43`` on top of ``environment.py:26-213``) for B environments at once: ``reset`` / ``step`` /
``set_agent_state`` + ``observe`` with the reference's observation dictionary (``internal`` [B, 14], ``external``
[B, 32], float32), reward and termination flags.  All per-step work -- robot and obstacle motion, collision and goal
flags, sector / ray observation with memory, path observations, reward -- is ONE HIP kernel launch
(``csrc/envgpu.hip``); this module only prepares the maps once (padded outlines, key frames, path lengths -> one record
of doubles per environment) and keeps the state tensors.  torch is used for device memory only.

``BatchedImgsEnv`` is the image-observation variant (``variants/imgs_reward1.py``): the same step kernel plus an image kernel
(``csrc/envimg.hip``) that draws ``external`` as uint8 [B, 3, H, W].

Maps and reference paths are inputs (the reference gets the path from ``extremitypathfinder``, a third-party A*;
``environment.py:124-147``); ``path_plan.plan_reference_paths`` plans them on the GPU for drawn maps
(:func:`random_dynamic_spec`), and :meth:`BatchedRaysEnv.replace_maps` puts new maps into a running environment.  There is no
CPU path: without the built library and a HIP device construction raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import rl_geometry as rg
from .solver import MpcGpuError, bind_exports, load_library

STATE_DOUBLES = 32
N_INTERNAL = 14
N_EXTERNAL = 32
HDR = 16

# MobileRobotSpecification (agent.py:7-16)
ROBOT = dict(radius=0.5, speed_min=-0.5, speed_max=1.5, angvel_min=-0.5, angvel_max=0.5, acc_min=-1.0, acc_max=1.0,
             angacc_min=-3.0, angacc_max=3.0)


def _f32(a) -> np.ndarray:
    """Round through float32 the way the reference's ``np.float32`` node / key-frame arrays do."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def static_obstacle(nodes: Sequence[Sequence[float]], radius: float = ROBOT["radius"]) -> Dict:
    """``Obstacle.create_mpc_static`` (obstacle.py:189-191): polygon padded by the robot radius, no motion."""
    padded = _f32(rg.buffer_polygon(_f32(rg.orient(nodes)), radius))
    return dict(padded_nodes=padded, time_steps=[0.0, 1.0], keyframes=[(0.0, 0.0, 0.0)], interp="linear", offset=0.0)


def periodic_obstacle(p1, p2, freq: float, rx: float, ry: float, angle: float, corners: int = 12,
                      radius: float = ROBOT["radius"]) -> Dict:
    """``Obstacle.create_mpc_dynamic`` (obstacle.py:193-201): an ellipse-like polygon oscillating between ``p1`` and
    ``p2`` with cosine easing (``Animation.periodic``, obstacle.py:97-105)."""
    padded = _f32(rg.buffer_polygon(_f32(rg.ellipse_nodes(rx, ry, corners)), radius))
    step = math.pi / freq if freq != 0 else 1.0
    p1, p2 = _f32(p1), _f32(p2)
    # Reference quirk, kept: the loop that builds the nodes re-uses the name ``angle`` (obstacle.py:196-198), so the
    # key frames are created with the LAST node angle 2 pi (corners - 1) / corners, not with the caller's ``angle``.
    rot = 2.0 * math.pi * (corners - 1) / corners if corners > 0 else angle
    return dict(padded_nodes=padded, time_steps=[0.0, step, step],
                keyframes=[(p1[0], p1[1], rot), (p2[0], p2[1], rot)], interp="cosine", offset=0.0)


def keyframe_pose(obstacle: Dict, time: float):
    """(x, y, rotation) of an obstacle at ``time``: the cyclic key-frame animation of ``obstacle.py:71-88`` (host-side
    twin of what the kernel evaluates per step; used by callers that need obstacle positions, e.g. the MPC feeders)."""
    steps, frames = obstacle["time_steps"], obstacle["keyframes"]
    tm = (time + obstacle["offset"]) % float(sum(steps))
    t = 0.0
    for i in range(len(frames)):
        t += steps[i]
        if t <= tm < t + steps[i + 1]:
            x = (tm - t) / steps[i + 1]
            alpha = (1.0 - math.cos(x * math.pi)) / 2.0 if obstacle["interp"] == "cosine" else x
            k0, k1 = frames[i], frames[(i + 1) % len(frames)]
            return tuple(k0[j] * (1.0 - alpha) + k1[j] * alpha for j in range(3))
    return tuple(frames[-1])


def make_map(boundary, static: Sequence, dynamic: Sequence[Dict], start, goal, path,
             radius: float = ROBOT["radius"]) -> Dict:
    """Map description -> the spec both the record packer and ``oracle/rl_env_numpy.py`` consume."""
    obstacles = [static_obstacle(n, radius) for n in static]
    obstacles += [periodic_obstacle(radius=radius, **d) for d in dynamic]
    return dict(start=np.asarray(start, dtype=np.float64), goal=_f32(goal)[:2],
                path=np.asarray(path, dtype=np.float64).reshape(-1, 2),
                boundary_padded=rg.buffer_polygon(_f32(rg.orient(boundary)), -radius), obstacles=obstacles)


def random_dynamic_spec(rng) -> Dict:
    """``generate_map_dynamic`` (utils/map.py:158-189) on a numpy ``Generator``: a 40 x 20 m hall, three static boxes and
    seven periodic obstacles, start on x = 5 and goal on x = 35.  The same distributions in the same order of draws, not
    the same stream as Python's ``random``.  Returns the keyword form of :func:`make_map` without ``path`` (the boxes may
    overlap and may cross the boundary; ``path_plan.plan_reference_paths`` plans a path or says there is none)."""
    start = [5.0, float(rng.uniform(5, 15)), float(rng.uniform(0, 2 * math.pi)), 0.0, 0.0]
    static, dynamic = [], []
    for i in range(10):
        x, y = float(rng.uniform(10, 30)), float(rng.uniform(0, 20))
        if i < 3:
            w = max(4.0, float(rng.uniform(0, 0.5 * min(x - 10, 30 - x))))
            h = max(4.0, float(rng.uniform(0, min(y, 20 - y))))
            x0, y0 = x - w / 2, y - h / 2
            static.append([(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)])
        else:
            x2, y2 = x + float(rng.uniform(-5, 5)), y + float(rng.uniform(-5, 5))
            rx, ry = float(rng.uniform(0.2, 1.2)), float(rng.uniform(0.2, 1.2))
            freq, angle = float(rng.uniform(0.3, 0.7)), float(rng.uniform(0, 2 * math.pi))
            dynamic.append(dict(p1=(x, y), p2=(x2, y2), freq=freq, rx=rx, ry=ry, angle=angle))
    return dict(boundary=[(0.0, 0.0), (40.0, 0.0), (40.0, 20.0), (0.0, 20.0)], static=static, dynamic=dynamic, start=start,
                goal=[35.0, float(rng.uniform(5, 15))])


class _CParams(C.Structure):
    _fields_ = [("n_path_max", C.c_int32), ("n_obst_max", C.c_int32), ("n_kf_max", C.c_int32), ("n_edge_max", C.c_int32),
                ("num_segments", C.c_int32), ("corner_samples", C.c_int32),
                ("time_step", C.c_double), ("sample_offset", C.c_double), ("collision_factor", C.c_double),
                ("reach_goal_factor", C.c_double), ("cross_track_factor", C.c_double),
                ("excessive_speed_factor", C.c_double), ("reference_speed", C.c_double),
                ("path_progress_factor", C.c_double),
                ("radius", C.c_double), ("speed_min", C.c_double), ("speed_max", C.c_double), ("angvel_min", C.c_double),
                ("angvel_max", C.c_double), ("acc_min", C.c_double), ("acc_max", C.c_double), ("angacc_min", C.c_double),
                ("angacc_max", C.c_double)]


class _CImgParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("down_sample", C.c_int32), ("reserved", C.c_int32),
                ("scale_x", C.c_double), ("scale_y", C.c_double), ("center_x", C.c_double), ("center_y", C.c_double),
                ("angle", C.c_double)]


_VP, _I32, _PP, _IP = C.c_void_p, C.c_int32, C.POINTER(_CParams), C.POINTER(_CImgParams)
# export -> (restype, argtypes); include/mpcgpu_env.h
_ENV_TABLE = {
    "mpcgpu_env_record_doubles": (_I32, [_PP]),
    "mpcgpu_env_step_dev": (_I32, [_I32, _PP, _I32] + [_VP] * 8),
    "mpcgpu_env_step_autoreset_dev": (_I32, [_I32, _PP, _I32] + [_VP] * 10 + [_I32, _VP]),
    "mpcgpu_env_last_error": (C.c_char_p, []),
    "mpcgpu_env_img_state_doubles": (_I32, [_IP]),
    "mpcgpu_env_step_imgs_dev": (_I32, [_I32, _PP, _IP, _I32] + [_VP] * 10),
    "mpcgpu_env_step_imgs_autoreset_dev": (_I32, [_I32, _PP, _IP, _I32] + [_VP] * 12 + [_I32, _VP]),
}
ENV_EXPORTS = tuple(_ENV_TABLE)


def _bind(lib):
    return bind_exports(lib, "env", _ENV_TABLE, "csrc/envgpu.hip, csrc/envimg.hip")


def path_lengths(path: np.ndarray):
    """(cumulative length per node, length per segment), summed sequentially in float64 so that
    ``cum[i + 1] == cum[i] + seg[i]`` holds exactly (projection onto a node and the corner search must agree)."""
    n = len(path)
    cum, seg = np.zeros(n), np.zeros(n)
    for i in range(n - 1):
        seg[i] = math.sqrt((path[i + 1][0] - path[i][0]) ** 2 + (path[i + 1][1] - path[i][1]) ** 2)
        cum[i + 1] = cum[i] + seg[i]
    return cum, seg


def pack_records(maps: Sequence[Dict], n_kf_max: int = 2, limits: Optional[Dict] = None):
    """maps -> (records [B, R] float64, dict of the batch maxima P, M, K, E); layout: include/mpcgpu_env.h.

    ``limits`` (``n_path_max``, ``n_obst_max``, ``n_kf_max``, ``n_edge_max`` of an existing record table) packs the maps
    into THAT table's layout instead of the batch's own, and raises if a map does not fit."""
    P = max(2, max(len(m["path"]) for m in maps))
    M = max(len(m["obstacles"]) for m in maps)
    K = max([n_kf_max] + [len(o["keyframes"]) for m in maps for o in m["obstacles"]])
    E = max(len(m["boundary_padded"]) + sum(len(o["padded_nodes"]) for o in m["obstacles"]) for m in maps)
    if limits is not None:
        need = dict(n_path_max=P, n_obst_max=M, n_kf_max=K, n_edge_max=E)
        over = [f"{k} {need[k]} > {limits[k]}" for k in need if need[k] > limits[k]]
        if over:
            raise ValueError("a map does not fit the record table: " + ", ".join(over))
        P, M, K, E = (int(limits[k]) for k in ("n_path_max", "n_obst_max", "n_kf_max", "n_edge_max"))
    if P > 64 or M > 31 or K > 4:
        raise ValueError("limits: at most 64 path nodes, 31 obstacles, 4 key frames per obstacle")
    an = 4 + (K + 1) + 3 * K
    o_cum, o_len, o_xy = HDR, HDR + P, HDR + 2 * P
    o_anim = o_xy + 2 * P
    o_edge = o_anim + M * an
    R = o_edge + 5 * E
    R += R & 1
    rec = np.zeros((len(maps), R))
    for b, m in enumerate(maps):
        r = rec[b]
        path = np.asarray(m["path"], dtype=np.float64)
        cum, seg = path_lengths(path)
        n = len(path)
        r[0], r[1], r[3], r[4] = n, len(m["obstacles"]), m["goal"][0], m["goal"][1]
        r[5:10] = np.asarray(m["start"], dtype=np.float64)
        r[o_cum:o_cum + n], r[o_len:o_len + n] = cum, seg
        r[o_xy:o_xy + 2 * n] = path.reshape(-1)
        edges = []
        ring = np.asarray(m["boundary_padded"], dtype=np.float64)
        edges += [(*ring[i], *ring[(i + 1) % len(ring)], -1.0) for i in range(len(ring))]
        for j, ob in enumerate(m["obstacles"]):
            a = r[o_anim + j * an:o_anim + (j + 1) * an]
            nk = len(ob["keyframes"])
            a[0] = 1.0 if ob["interp"] == "cosine" else 0.0
            a[1], a[2], a[3] = ob["offset"], nk, float(sum(ob["time_steps"]))
            a[4:4 + nk + 1] = ob["time_steps"]
            a[4 + K + 1:4 + K + 1 + 3 * nk] = np.asarray(ob["keyframes"], dtype=np.float64).reshape(-1)
            ring = np.asarray(ob["padded_nodes"], dtype=np.float64)
            edges += [(*ring[i], *ring[(i + 1) % len(ring)], float(j)) for i in range(len(ring))]
        r[2] = len(edges)
        blk = np.full((E, 5), 0.0)
        blk[:, 4] = -2.0
        blk[:len(edges)] = np.asarray(edges)
        r[o_edge:o_edge + 5 * E] = blk.reshape(-1)
    return rec, dict(n_path_max=P, n_obst_max=M, n_kf_max=K, n_edge_max=E)


def _over(mask, like):
    """A row mask [B] shaped to broadcast over ``like`` [B, ...]."""
    return mask.reshape((-1,) + (1,) * (like.dim() - 1))


class BatchedRaysEnv:
    """B independent ``TrajectoryPlannerEnvironmentRaysReward1`` environments stepped by one kernel launch.

    ``maps``: one spec per environment (:func:`make_map`).  Observations / rewards / flags are torch tensors on the
    device.  ``max_episode_steps`` is the gym ``TimeLimit`` the reference registers (environment/__init__.py:15-25)."""

    def __init__(self, maps: Sequence[Dict], device: int = 0, time_step: float = 0.2, max_episode_steps: int = 1000,
                 sample_offset: float = 0.0, collision_factor: float = 4.0, reach_goal_factor: float = 3.0,
                 cross_track_factor: float = 0.05, reference_speed: float = ROBOT["speed_max"] * 0.8,
                 path_progress_factor: float = 2.0, capacity: Optional[Dict] = None):
        """``capacity`` (``n_path_max``, ``n_obst_max``, ``n_kf_max``, ``n_edge_max``) sizes the record table for maps that
        come later (:meth:`replace_maps`, :meth:`load_spares`) instead of for ``maps`` alone; ``maps`` must fit it."""
        import torch
        if not torch.cuda.is_available():
            raise MpcGpuError("BatchedRaysEnv needs a HIP device: the environment step is a GPU kernel, there is no CPU path")
        self._torch = torch
        self._lib = _bind(load_library())
        self.device = torch.device("cuda", device)
        self.device_index = device
        self.B = len(maps)
        rec, maxima = pack_records(maps, limits=capacity)
        self.params = _CParams(num_segments=8, corner_samples=3, time_step=time_step, sample_offset=sample_offset,
                               collision_factor=collision_factor, reach_goal_factor=reach_goal_factor,
                               cross_track_factor=cross_track_factor, excessive_speed_factor=2.0 * path_progress_factor,
                               reference_speed=reference_speed, path_progress_factor=path_progress_factor,
                               **maxima, **ROBOT)
        R = self._lib.mpcgpu_env_record_doubles(C.byref(self.params))
        if R != rec.shape[1]:
            raise MpcGpuError(f"record layout mismatch: library {R} doubles, packer {rec.shape[1]} "
                              f"({self._lib.mpcgpu_env_last_error().decode()})")
        self.records = torch.from_numpy(rec).to(self.device)
        start = np.stack([np.asarray(m["start"], dtype=np.float64) for m in maps])
        self._start = torch.from_numpy(start).to(self.device)
        self.state = torch.zeros(self.B, STATE_DOUBLES, dtype=torch.float64, device=self.device)
        self.obs_internal = torch.zeros(self.B, N_INTERNAL, dtype=torch.float32, device=self.device)
        self.obs_external = torch.zeros(self.B, N_EXTERNAL, dtype=torch.float32, device=self.device)
        self.reward = torch.zeros(self.B, dtype=torch.float64, device=self.device)
        self.terminated = torch.zeros(self.B, dtype=torch.uint8, device=self.device)
        self.truncated = torch.zeros(self.B, dtype=torch.uint8, device=self.device)
        self.term_internal = torch.zeros_like(self.obs_internal)
        self.term_external = torch.zeros_like(self.obs_external)
        self.max_episode_steps = max_episode_steps
        self.time_step = time_step
        self.records2 = None     # [2, B, R] once enable_spares() ran; self.records is then its table 0

    # ---- a spare record per row: map turnover inside the auto-reset step (include/mpcgpu_map.h) --------------------
    def _limits(self) -> Dict:
        return {k: int(getattr(self.params, k)) for k in ("n_path_max", "n_obst_max", "n_kf_max", "n_edge_max")}

    def enable_spares(self) -> None:
        """Give every row a second record.  From now on ``step(actions, auto_reset=True)`` launches the fresh-map variant
        of the step kernel: a row whose episode ends while its spare is ready (:meth:`load_spares`) starts the next
        episode on the spare inside that launch -- counted in ``loaded`` -- and otherwise resets on the map it has --
        counted in ``stale``.  ``which`` [B] says which of the two tables a row is on; ``reset``, ``observe``,
        ``replace_maps`` and the step without auto-reset act on that table.  Device memory: a second table of B * R
        doubles (R = ``records.shape[1]``) and four int32 vectors of B."""
        if self.records2 is not None:
            return
        from . import map_stream
        map_stream._bind(self._lib)
        torch = self._torch
        self.records2 = torch.stack([self.records, self.records]).contiguous()
        self.records = self.records2[0]
        for name in ("which", "spare_ready", "loaded", "stale"):
            setattr(self, name, torch.zeros(self.B, dtype=torch.int32, device=self.device))
        self._rows = torch.arange(self.B, device=self.device)

    def enable_fresh_maps(self, seed: int = 0, refill_every: int = 16) -> None:
        """A new random map per episode, drawn, planned and packed on the device (``map_stream``, ``csrc/mapgpu.hip``):
        :meth:`enable_spares`, then every ``refill_every``-th ``step(actions, auto_reset=True)`` enqueues a refill behind the
        step -- for the rows whose spare is missing: draw map ``b + B * attempt[b]`` of stream ``seed``
        (``map_stream.spec_of``), inflate its outlines, plan its reference path (``csrc/plangpu.hip``) and pack the record
        into the spare slot.  A row whose draw has no path, or does not fit, draws again at the next refill.  Nothing
        synchronises with the host.  The default ``refill_every`` is the largest of 1, 4, 8, 16, 32 without a stale reset
        in 2000 steps of random actions at B = 4096 (``profiles/map_stream_bench.txt``).  ``refill_status`` [B] keeps ``map_stream.STATUS`` of the last refill.  Raises
        ``ValueError``, before anything is allocated, if the record table is smaller than ``map_stream.DYNAMIC_CAPACITY``
        (build the environment with ``capacity=map_stream.DYNAMIC_CAPACITY``).  Extra device memory: the second record
        table (B * R doubles), the spec (288), ring (396) and path (130) tables of B rows, and six int32 vectors."""
        from . import map_stream, path_plan
        short = [k for k, v in map_stream.DYNAMIC_CAPACITY.items() if getattr(self.params, k) < v]
        if short:
            raise ValueError("the record table is smaller than map_stream.DYNAMIC_CAPACITY in " + ", ".join(short))
        if int(refill_every) < 1:
            raise ValueError("refill_every must be at least 1")
        self.enable_spares()
        torch = self._torch
        self.fresh_seed, self.refill_every = int(seed), int(refill_every)
        self.attempt = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.refill_status = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self._spec = torch.zeros(self.B, map_stream.SPEC_DOUBLES, dtype=torch.float64, device=self.device)
        self._planner = path_plan.PathPlanner(self.device_index)
        self._calls = 0
        self._rings = self._plan = None     # ring records, start / goal and planner output: allocated by the first refill
        self.refill()

    def refill(self) -> None:
        """Enqueue one refill of the missing spares on the current stream (draw, rings, plan, record: four launches)."""
        from . import map_stream
        map_stream.draw_specs_dev(self._spec, self.spare_ready, self.attempt, self.fresh_seed, self.device_index)
        self._rings = rings, start_goal = map_stream.rings_dev(self._spec, self.spare_ready, self.device_index, out=self._rings)
        self._plan = self._planner.plan_dev(rings, start_goal, map_stream.VERT_MAX, map_stream.RING_MAX, out=self._plan)
        status, n_nodes, nodes, _ = self._plan
        map_stream.records_dev(self.params, self._spec, status, n_nodes, nodes, self.records2, self.which, self.spare_ready,
                               self.refill_status, self.device_index)

    def load_spares(self, rows, maps: Sequence[Dict]) -> None:
        """Pack ``maps`` (:func:`make_map`) into the spare records of ``rows`` and mark them ready; a spare that was ready
        is replaced.  Raises ``ValueError``, before anything is written, if a map does not fit the table.  Enqueued on
        the current stream, like the step that will read them."""
        torch = self._torch
        if self.records2 is None:
            raise MpcGpuError("load_spares needs enable_spares() first")
        rows = [int(r) for r in rows]
        if len(rows) != len(maps) or len(set(rows)) != len(rows) or any(r < 0 or r >= self.B for r in rows):
            raise ValueError(f"load_spares needs one map per row, rows distinct and in [0, {self.B})")
        if not rows:
            return
        rec, _ = pack_records(maps, limits=self._limits())
        idx = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
        self.records2[1 - self.which[idx].long(), idx] = torch.from_numpy(rec).to(self.device)
        self.spare_ready[idx] = 1

    def current_records(self):
        """[B, R] copy of the record every row is on."""
        if self.records2 is None:
            return self.records.clone()
        return self.records2[self.which.long(), self._rows]

    def replace_maps(self, rows, maps: Sequence[Dict]) -> None:
        """Give environments ``rows`` the new ``maps`` (:func:`make_map`, e.g. with a path of ``path_plan``): their rows
        of the device record table are re-packed in place, no other row is touched.  Raises ``ValueError``, before
        anything is written, if a map exceeds the table's ``n_path_max``, ``n_obst_max``, ``n_kf_max`` or
        ``n_edge_max``.  The rows keep their state until a following ``reset(mask)`` starts them on the new maps.  After
        :meth:`enable_spares` it is the record a row is ON that is replaced; its spare is left alone."""
        torch = self._torch
        rows = [int(r) for r in rows]
        if len(rows) != len(maps) or len(set(rows)) != len(rows) or any(r < 0 or r >= self.B for r in rows):
            raise ValueError(f"replace_maps needs one map per row, rows distinct and in [0, {self.B})")
        if not rows:
            return
        rec, _ = pack_records(maps, limits=self._limits())
        assert rec.shape[1] == self.records.shape[1]
        idx = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
        start = np.stack([np.asarray(m["start"], dtype=np.float64) for m in maps])
        if self.records2 is not None:
            self.records2[self.which[idx].long(), idx] = torch.from_numpy(rec).to(self.device)
            return                                  # the start state is read from the current record
        self.records[idx] = torch.from_numpy(rec).to(self.device)
        self._start[idx] = torch.from_numpy(start).to(self.device)

    # ---- what the image variant describes differently ---------------------------------------------------------------
    _EXTERNAL = ("obs_external", "term_external")    # attributes: the external observation and its terminal copy
    _ROW_STATE = ("state",)                          # per-row state tensors, saved in state_dict under these names ...
    _RESET_CLEARS = ()                               # ... and those of them a reset zeroes for the rows it resets
    _ENTRIES = ("mpcgpu_env_step_dev", "mpcgpu_env_step_autoreset_dev", "mpcgpu_env_step_fresh_dev")

    def _args(self, table: tuple, aptr, max_steps) -> tuple:
        """The arguments of a C entry but the stream: ``table`` are the pointers of the record table (and of the spare
        vectors with it), ``max_steps`` is None for the plain entry, which ends after ``terminated``."""
        tail = () if max_steps is None else (self.truncated.data_ptr(), self.term_internal.data_ptr(),
                                             self.term_external.data_ptr(), max_steps)
        return (self.device_index, C.byref(self.params), self.B, *table, self.state.data_ptr(), aptr,
                self.obs_internal.data_ptr(), self.obs_external.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                *tail)

    # ---- kernel launch ---------------------------------------------------------------------------------------------
    def _launch(self, actions, max_steps: int = 0) -> None:
        """Enqueue one step on the current stream: the fresh-table entry once :meth:`enable_spares` ran, otherwise the
        auto-reset entry when ``max_steps > 0``, otherwise the plain one.  ``actions=None`` observes (no auto-reset
        then)."""
        torch = self._torch
        aptr = None
        if actions is not None:
            actions = torch.as_tensor(actions, dtype=torch.int32, device=self.device).contiguous()
            if actions.shape != (self.B,):
                raise ValueError(f"actions must have shape ({self.B},)")
            aptr = actions.data_ptr()
        plain, autoreset, fresh = self._ENTRIES
        if self.records2 is not None:
            entry, table = fresh, (self.records2.data_ptr(), self.which.data_ptr(), self.spare_ready.data_ptr(),
                                   self.loaded.data_ptr(), self.stale.data_ptr())
        else:
            entry, table = (autoreset if max_steps > 0 else plain), (self.records.data_ptr(),)
        rc = getattr(self._lib, entry)(*self._args(table, aptr, None if entry == plain else int(max_steps)),
                                       torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise MpcGpuError(self._lib.mpcgpu_env_last_error().decode())

    def _obs(self) -> Dict[str, "object"]:
        return {"internal": self.obs_internal.clone(), "external": getattr(self, self._EXTERNAL[0]).clone()}

    # ---- gym-style API ---------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """Reset all (or the masked) environments to their map's start state (environment.py:166-186); the image
        variant clears their image history first (environment.py:161-180).  The observation memory is NOT cleared: the
        reference's component keeps ``old_obs`` across episodes."""
        torch = self._torch
        if mask is None:
            mask = torch.ones(self.B, dtype=torch.bool, device=self.device)
        mask = torch.as_tensor(mask, device=self.device).bool()
        fresh = torch.zeros_like(self.state)
        fresh[:, :5] = self._start if self.records2 is None else self.records2[self.which.long(), self._rows, 5:10]
        fresh[:, 8:24] = self.state[:, 8:24]
        self.state = torch.where(_over(mask, fresh), fresh, self.state)
        # update_status(reset=True) + get_observation for the reset rows only: the launch observes every environment, so the
        # rows that are NOT reset get their state, observation (including its one-step memory half), reward and
        # termination flag restored afterwards -- a partial reset must leave them bit-identical
        outputs = ("obs_internal", self._EXTERNAL[0], "reward", "terminated")
        kept = {name: getattr(self, name).clone() for name in self._ROW_STATE + outputs}
        for name in self._RESET_CLEARS:
            setattr(self, name, torch.where(_over(mask, kept[name]), torch.zeros_like(kept[name]), kept[name]))
        self._launch(None)
        for name in self._ROW_STATE:
            setattr(self, name, torch.where(_over(mask, kept[name]), getattr(self, name), kept[name]))
        self.state[:, 6] = torch.where(mask, torch.zeros_like(self.state[:, 6]), self.state[:, 6])
        for name in outputs:
            getattr(self, name).copy_(torch.where(_over(mask, kept[name]), getattr(self, name), kept[name]))
        return self._obs()

    def _saved(self) -> tuple:
        return self._ROW_STATE + ("obs_internal", self._EXTERNAL[0], "reward", "terminated", "truncated")

    def state_dict(self) -> Dict:
        """Everything a continuation needs: robot / clock state (incl. the one-step observation memory kept in it; the image
        history of the image variant) and the observation, reward and flags of the last launch."""
        d = {name: getattr(self, name).clone() for name in self._saved()}
        if self.records2 is not None:
            # maps change while the environment runs: both record tables (2 * B * R doubles, R = records.shape[1]; 16 * B * R
            # bytes) and the per-row vectors belong to the state
            d.update({k: getattr(self, k).clone() for k in self._FRESH_KEYS if getattr(self, k, None) is not None})
            if getattr(self, "refill_every", 0):
                d["refill_calls"] = self._calls
        return d

    _FRESH_KEYS = ("records2", "which", "spare_ready", "loaded", "stale", "attempt")

    def load_state_dict(self, d: Dict) -> None:
        if ("records2" in d) != (self.records2 is not None):
            raise ValueError("state_dict and environment differ in enable_spares()")
        for k in self._saved():
            getattr(self, k).copy_(d[k].to(self.device))
        if self.records2 is not None:
            for k in self._FRESH_KEYS:
                if k in d and getattr(self, k, None) is not None:
                    getattr(self, k).copy_(d[k].to(self.device))
            if getattr(self, "refill_every", 0):
                self._calls = int(d.get("refill_calls", 0))

    def step(self, actions, auto_reset: bool = False):
        """``env.step`` (environment.py:199-213) -> (obs, reward [B], terminated [B] bool, truncated [B] bool, info).

        ``auto_reset=True`` is the vectorised-environment behaviour (SB3 VecEnv + gym TimeLimit): ended episodes are reset
        INSIDE the same kernel launch, ``obs`` is then the first observation of the next episode and
        ``info["terminal_observation"]`` the one the episode ended in (for the other rows it equals ``obs``)."""
        torch = self._torch
        if not auto_reset:
            self._launch(actions)
            obs = self._obs()
            terminated = self.terminated.bool()
            truncated = (self.state[:, 25] >= self.max_episode_steps) & ~terminated
            return obs, self.reward.clone(), terminated, truncated, {"success": (self.state[:, 7].to(torch.int64) & 4) != 0}
        if int(self.max_episode_steps) <= 0:
            # the library's own refusal of the auto-reset entry, in its words; made here because _launch, and the fresh entry
            # itself, read max_steps = 0 as "no auto-reset"
            raise MpcGpuError("max_episode_steps must be positive")
        self._launch(actions, int(self.max_episode_steps))
        self._count_autoreset_steps(1)
        return self._autoreset_result()

    def _count_autoreset_steps(self, n: int) -> None:
        """The refill cadence of :meth:`enable_fresh_maps`, behind the launch or launches that made ``n`` auto-reset steps (see
        include/mpcgpu_map.h): ONE refill if the count of steps passed a multiple of ``refill_every``.  ``n = 1`` is every
        ``refill_every``-th step; a launch of ``n`` steps (``collect_fresh.collect_rays_fresh``) is followed by at most one
        refill, since a second one would find the same rows missing."""
        if getattr(self, "refill_every", 0):
            before = self._calls
            self._calls += int(n)
            if before // self.refill_every != self._calls // self.refill_every:
                self.refill()

    def _autoreset_result(self):
        torch = self._torch
        obs = self._obs()
        terminated, truncated = self.terminated.bool(), self.truncated.bool()
        done = terminated | truncated
        term_external = getattr(self, self._EXTERNAL[1])
        # state[7] already belongs to the next episode where a reset happened; state[26] keeps this step's flags
        info = {"success": (self.state[:, 26].to(torch.int64) & 4) != 0,
                "terminal_observation": {"internal": torch.where(_over(done, self.term_internal), self.term_internal, obs["internal"]),
                                         "external": torch.where(_over(done, term_external), term_external, obs["external"])}}
        return obs, self.reward.clone(), terminated, truncated, info

    def set_agent_state(self, states) -> None:
        """``set_agent_state`` (environment.py:189-193) for every environment: rows of (x, y, theta, v, w)."""
        torch = self._torch
        self.state[:, :5] = torch.as_tensor(states, dtype=torch.float64, device=self.device)

    def observe(self):
        """``update_status(reset=False)`` + ``get_observation()`` without moving anything (src/main.py:181-189)."""
        self._launch(None)
        return self._obs()

    # ---- convenience -------------------------------------------------------------------------------------------------
    @property
    def agent_state(self):
        return self.state[:, :5]

    @property
    def path_progress(self):
        return self.state[:, 24]

    @property
    def flags(self):
        """[B, 3] bool: collided with obstacle, collided with boundary, reached goal."""
        f = self.state[:, 7].to(self._torch.int64)
        return self._torch.stack([(f & 1) != 0, (f & 2) != 0, (f & 4) != 0], dim=1)


# ----------------------------------------------------------------------------------------------------------------------
# image-observation variant (variants/imgs_reward1.py, components/ext_obsv_image.py)
# ----------------------------------------------------------------------------------------------------------------------
def image_params(width: int = 54, height: int = 54, scale_x: float = 1 / 18, scale_y: float = 1 / 18, down_sample: int = 2,
                 center_x: float = 0.5, center_y: float = 0.3, angle: float = 0.0) -> _CImgParams:
    """The image keyword arguments of ``TrajectoryPlannerEnvironmentImgsReward1`` (imgs_reward1.py:17-24) as the C struct."""
    if down_sample != int(down_sample):
        raise ValueError("only down_sample = 2 is built")
    return _CImgParams(width=int(width), height=int(height), down_sample=int(down_sample), scale_x=scale_x, scale_y=scale_y,
                       center_x=center_x, center_y=center_y, angle=angle)


def image_distance_field(width: int = 54, height: int = 54, scale_x: float = 1 / 18, scale_y: float = 1 / 18,
                         center_x: float = 0.5, center_y: float = 0.3) -> np.ndarray:
    """Channel 2 of the image observation, uint8 [height, width]: ext_obsv_image.py:42-50, computed once on the host (it
    depends on the image parameters only) and copied into every observation by the kernel."""
    w = (width - 1) / (scale_x * width)
    h = (height - 1) / (scale_y * height)
    x, y = np.meshgrid(np.linspace(-w * center_x, w * (1 - center_x), width),
                       np.linspace(-h * center_y, h * (1 - center_y), height))
    distance = 2 / (1 + np.exp(-2 * np.sqrt(x ** 2 + y ** 2) / 10)) - 1   # components/utils.py:10-15
    distance = distance - np.min(distance)
    return (255.5 * (1 - distance / np.max(distance))).astype(np.uint8)


class BatchedImgsEnv(BatchedRaysEnv):
    """B independent ``TrajectoryPlannerEnvironmentImgsReward1`` environments (variants/imgs_reward1.py:7-49).

    Robot, obstacles, internal observation, reward, flags and episode bookkeeping are those of :class:`BatchedRaysEnv`
    (the same step kernel); the external observation is the image of ``components/ext_obsv_image.py``, uint8
    ``[B, 3, H, W]``, drawn by a second kernel (``csrc/envimg.hip``): the padded boundary at 255 with the obstacles at 0,
    at the current clock (channel 0) and at the oldest of the last 6 observations since the reset (channel 1), and the
    constant distance field (channel 2).  Every observation pushes that history -- steps, ``observe()``, resets -- and a
    reset clears it first (environment.py:161-180).

    ``map_turnover=True`` builds the environment for a new map per episode (``include/mpcgpu_map.h``,
    ``mpcgpu_env_step_imgs_fresh_dev``): :meth:`enable_spares` / :meth:`enable_fresh_maps`, ``load_spares``, ``refill`` and
    ``current_records`` then work as on :class:`BatchedRaysEnv`.  A row that turns over gets its terminal image from the
    map its episode ended on and its next observation from the new one.  ``capacity`` sizes the record table for the
    maps to come; its ``n_edge_max`` must fit the image kernel's edge staging in LDS, which is checked here."""

    is_image_env = True

    def __init__(self, maps: Sequence[Dict], device: int = 0, time_step: float = 0.2, max_episode_steps: int = 1000,
                 sample_offset: float = 0.0, collision_factor: float = 4.0, reach_goal_factor: float = 3.0,
                 cross_track_factor: float = 0.05, reference_speed: float = ROBOT["speed_max"] * 0.8,
                 path_progress_factor: float = 2.0, image_width: int = 54, image_height: int = 54,
                 image_scale_x: float = 1 / 18, image_scale_y: float = 1 / 18, image_down_sample: int = 2,
                 image_center_x: float = 0.5, image_center_y: float = 0.3, image_angle: float = 0.0,
                 capacity: Optional[Dict] = None, map_turnover: bool = False):
        lib = _bind(load_library())
        self.map_turnover = bool(map_turnover)
        self.img_params = image_params(image_width, image_height, image_scale_x, image_scale_y, image_down_sample,
                                       image_center_x, image_center_y, image_angle)
        n_img = lib.mpcgpu_env_img_state_doubles(C.byref(self.img_params))
        if n_img < 0:
            raise ValueError(lib.mpcgpu_env_last_error().decode())
        super().__init__(maps, device=device, time_step=time_step, max_episode_steps=max_episode_steps,
                         sample_offset=sample_offset, collision_factor=collision_factor, reach_goal_factor=reach_goal_factor,
                         cross_track_factor=cross_track_factor, reference_speed=reference_speed,
                         path_progress_factor=path_progress_factor, capacity=capacity)
        torch = self._torch
        H, W = int(image_height), int(image_width)
        self.image_shape = (3, H, W)
        self.img_state = torch.zeros(self.B, n_img, dtype=torch.float64, device=self.device)
        self.obs_image = torch.zeros(self.B, 3, H, W, dtype=torch.uint8, device=self.device)
        self.term_image = torch.zeros_like(self.obs_image)
        self.distance_field = torch.from_numpy(image_distance_field(W, H, image_scale_x, image_scale_y, image_center_x,
                                                                    image_center_y)).to(self.device).contiguous()
        if self.map_turnover:
            # a launch of no rows: the library validates the layout -- n_edge_max against the image kernel's LDS -- and
            # enqueues nothing
            rc = lib.mpcgpu_env_step_imgs_dev(self.device_index, C.byref(self.params), C.byref(self.img_params), 0,
                                              self.records.data_ptr(), self.state.data_ptr(), self.img_state.data_ptr(),
                                              self.distance_field.data_ptr(), None, self.obs_internal.data_ptr(),
                                              self.obs_image.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(), None)
            if rc != 0:
                raise ValueError(lib.mpcgpu_env_last_error().decode())

    _NO_TURNOVER = ("map turnover on the image environment is chosen at construction: build it with "
                    "BatchedImgsEnv(..., map_turnover=True) and a capacity= that holds the maps to come")

    def enable_spares(self) -> None:
        """As :meth:`BatchedRaysEnv.enable_spares`, for an environment built with ``map_turnover=True``: from now on every
        launch is ``mpcgpu_env_step_imgs_fresh_dev`` on the two-record table."""
        if not self.map_turnover:
            raise NotImplementedError(self._NO_TURNOVER)
        super().enable_spares()

    def enable_fresh_maps(self, seed: int = 0, refill_every: int = 16) -> None:
        """As :meth:`BatchedRaysEnv.enable_fresh_maps`, for an environment built with ``map_turnover=True``.  The default
        ``refill_every`` comes from the same rule, measured on this class: the largest of 1, 4, 8, 16, 32 without a stale
        reset in 2000 steps of random actions at B = 4096 (``tools/bench_maps.py --variant imgs``,
        ``profiles/img_fresh_bench.txt``: none up to 16, 0.4 % at 32) -- 16, as for the ray environment."""
        if not self.map_turnover:
            raise NotImplementedError(self._NO_TURNOVER)
        super().enable_fresh_maps(seed=seed, refill_every=refill_every)

    _EXTERNAL = ("obs_image", "term_image")
    _ROW_STATE = ("state", "img_state")
    _RESET_CLEARS = ("img_state",)               # the image history (environment.py:161-180)
    _ENTRIES = ("mpcgpu_env_step_imgs_dev", "mpcgpu_env_step_imgs_autoreset_dev", "mpcgpu_env_step_imgs_fresh_dev")

    def _args(self, table: tuple, aptr, max_steps) -> tuple:
        tail = () if max_steps is None else (self.truncated.data_ptr(), self.term_internal.data_ptr(),
                                             self.term_image.data_ptr(), max_steps)
        return (self.device_index, C.byref(self.params), C.byref(self.img_params), self.B, *table, self.state.data_ptr(),
                self.img_state.data_ptr(), self.distance_field.data_ptr(), aptr, self.obs_internal.data_ptr(),
                self.obs_image.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(), *tail)
