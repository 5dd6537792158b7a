"""Per-episode maps for the batched DRL environment: host side of ``include/mpcgpu_map.h``.

The reference draws a new map on every ``reset()`` (``src/pkg_dqn/environment/environment.py:161-169``).  Here every
environment row owns a current and a spare record, and the fresh-map variant of the auto-reset step
(``mpcgpu_env_step_fresh_dev``, ``BatchedRaysEnv.enable_spares``) moves a finished row onto its spare inside the launch;
``mpcgpu_env_step_imgs_fresh_dev`` is the same step for the image environment (``BatchedImgsEnv(map_turnover=True)``).

Maps are drawn from a COUNTER-BASED stream, so that map ``serial`` of stream ``seed`` can be regenerated from these two
numbers alone, on the host or on the device: :class:`CounterUniform` is a drop-in for the numpy ``Generator`` that
``rl_env.random_dynamic_spec`` takes, and ``map_draw_kernel`` (``csrc/mapgpu.hip``) makes the same 71 draws per map.

    u_k = (bits(seed, serial, k) >> 11) * 2**-53,        k = 0, 1, ...
    bits(seed, serial, k) = mix64(mix64(seed + G * serial) + G * (k + 1))        (all modulo 2**64)
    mix64 = the SplitMix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
    G = 0x9E3779B97F4A7C15
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np

from . import rl_env
from .solver import MpcGpuError, bind_exports

_VP, _I32, _PP = C.c_void_p, C.c_int32, C.POINTER(rl_env._CParams)
# export -> (restype, argtypes); include/mpcgpu_map.h
_MAP_TABLE = {
    "mpcgpu_env_step_fresh_dev": (_I32, [_I32, _PP, _I32] + [_VP] * 14 + [_I32, _VP]),
    "mpcgpu_env_step_imgs_fresh_dev": (_I32, [_I32, _PP, C.POINTER(rl_env._CImgParams), _I32] + [_VP] * 16 + [_I32, _VP]),
    "mpcgpu_map_spec_doubles": (_I32, []),
    "mpcgpu_map_draw_dev": (_I32, [_I32, _I32, C.c_uint64] + [_VP] * 4),
    "mpcgpu_map_rings_dev": (_I32, [_I32, _I32] + [_VP] * 5),
    "mpcgpu_map_record_dev": (_I32, [_I32, _PP, _I32] + [_VP] * 9),
    "mpcgpu_map_last_error": (C.c_char_p, []),
}
MAP_EXPORTS = tuple(_MAP_TABLE)

# Record-table capacity that holds EVERY generate_map_dynamic draw (derivation: include/mpcgpu_map.h).  Edges: the shrunk hall 4,
# three boxes of 4 corners x 5 points, seven convex 12-corner ellipses of at most 16 + 24 points: 4 + 60 + 280.  A path bends at
# box corners only: at most 2 + 12 nodes (16 leaves the record's path block a multiple of 8 doubles).
DYNAMIC_CAPACITY = dict(n_path_max=16, n_obst_max=10, n_kf_max=2, n_edge_max=344)
STATUS = {-1: "row skipped", 0: "ok", 1: "no path", 2: "start or goal not in free space", 3: "more than 64 path nodes",
          4: "malformed record", 5: "the map does not fit the record table"}

DRAWS_PER_MAP = 71
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)

# spec table (include/mpcgpu_map.h): one record of SPEC_DOUBLES doubles per map
MAX_BOUNDARY = 16     # boundary vertices
MAX_STATIC = 8        # static polygons
MAX_STATIC_VERTS = 10  # vertices of one static polygon
MAX_PERIODIC = 8      # periodic obstacles (12 corners each)
SPEC_HDR = 16
SPEC_BOUNDARY = SPEC_HDR
SPEC_STATIC = SPEC_BOUNDARY + 2 * MAX_BOUNDARY
SPEC_STATIC_STRIDE = 2 + 2 * MAX_STATIC_VERTS
SPEC_PERIODIC = SPEC_STATIC + MAX_STATIC * SPEC_STATIC_STRIDE
SPEC_PERIODIC_STRIDE = 8
SPEC_DOUBLES = SPEC_PERIODIC + MAX_PERIODIC * SPEC_PERIODIC_STRIDE
# capacities of the planner records the device writes: the boundary and every static polygon, each vertex bevelled into two
RING_MAX = 1 + MAX_STATIC
VERT_MAX = 2 * (MAX_BOUNDARY + MAX_STATIC * MAX_STATIC_VERTS)


def _mix64(z: np.uint64) -> np.uint64:
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


class CounterUniform:
    """``.uniform(lo, hi)`` of draw k = 0, 1, ... of map ``serial`` in stream ``seed`` (module docstring); ``.count`` is
    the number of draws made."""

    def __init__(self, seed: int, serial: int):
        with np.errstate(over="ignore"):
            self._key = _mix64(np.uint64(int(seed) % 2 ** 64) + _G * np.uint64(int(serial) % 2 ** 64))
        self.count = 0

    def bits(self, k: int) -> int:
        with np.errstate(over="ignore"):
            return int(_mix64(self._key + _G * np.uint64(k + 1)))

    def uniform(self, lo: float, hi: float) -> float:
        u = float(self.bits(self.count) >> 11) * 2.0 ** -53
        self.count += 1
        return lo + (hi - lo) * u


def spec_of(seed: int, serial: int) -> Dict:
    """Map ``serial`` of stream ``seed``: ``rl_env.random_dynamic_spec`` on the counter-based draws (71 of them)."""
    return rl_env.random_dynamic_spec(CounterUniform(seed, serial))


def pack_specs(specs: Sequence[Dict]) -> np.ndarray:
    """Specs in the keyword form of ``rl_env.make_map`` (``path`` not needed) -> spec table [n, SPEC_DOUBLES] float64,
    layout in ``include/mpcgpu_map.h``.  Raises ``ValueError`` before anything is written if a spec does not fit: more
    than 16 boundary vertices, 8 static polygons of 10 vertices, 8 periodic obstacles, or periodic obstacles with another
    corner count than 12."""
    rows = []
    for i, s in enumerate(specs):
        boundary = np.asarray(s["boundary"], dtype=np.float64).reshape(-1, 2)
        static = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in s["static"]]
        dynamic = list(s["dynamic"])
        if not 3 <= len(boundary) <= MAX_BOUNDARY:
            raise ValueError(f"spec {i}: {len(boundary)} boundary vertices, the spec table holds 3..{MAX_BOUNDARY}")
        if len(static) > MAX_STATIC or any(not 3 <= len(p) <= MAX_STATIC_VERTS for p in static):
            raise ValueError(f"spec {i}: the spec table holds {MAX_STATIC} static polygons of 3..{MAX_STATIC_VERTS} vertices")
        if len(dynamic) > MAX_PERIODIC or any(d.get("corners", 12) != 12 for d in dynamic):
            raise ValueError(f"spec {i}: the spec table holds {MAX_PERIODIC} periodic obstacles of 12 corners")
        if any(set(d) - {"p1", "p2", "freq", "rx", "ry", "angle", "corners"} for d in dynamic):
            raise ValueError(f"spec {i}: a periodic obstacle has keys the spec table does not hold")
        start = np.asarray(s["start"], dtype=np.float64).reshape(-1)
        goal = np.asarray(s["goal"], dtype=np.float64).reshape(-1)
        if len(start) != 5 or len(goal) < 2:
            raise ValueError(f"spec {i}: start needs 5 values and goal 2")
        rows.append((start, goal, boundary, static, dynamic))
    table = np.zeros((len(rows), SPEC_DOUBLES))
    for r, (start, goal, boundary, static, dynamic) in zip(table, rows):
        r[0:5], r[5:7] = start, goal[:2]
        r[7], r[8], r[9] = len(boundary), len(static), len(dynamic)
        r[SPEC_BOUNDARY:SPEC_BOUNDARY + 2 * len(boundary)] = boundary.reshape(-1)
        for j, p in enumerate(static):
            o = SPEC_STATIC + j * SPEC_STATIC_STRIDE
            r[o] = len(p)
            r[o + 2:o + 2 + 2 * len(p)] = p.reshape(-1)
        for j, d in enumerate(dynamic):
            o = SPEC_PERIODIC + j * SPEC_PERIODIC_STRIDE
            r[o:o + 8] = [d["p1"][0], d["p1"][1], d["p2"][0], d["p2"][1], d["freq"], d["rx"], d["ry"], d["angle"]]
    return table


def unpack_specs(table: np.ndarray):
    """The inverse of :func:`pack_specs` (a list of specs)."""
    out = []
    for r in np.asarray(table, dtype=np.float64).reshape(-1, SPEC_DOUBLES):
        nb, ns, nd = int(r[7]), int(r[8]), int(r[9])
        static, dynamic = [], []
        for j in range(ns):
            o = SPEC_STATIC + j * SPEC_STATIC_STRIDE
            static.append([tuple(map(float, q)) for q in r[o + 2:o + 2 + 2 * int(r[o])].reshape(-1, 2)])
        for j in range(nd):
            p = [float(x) for x in r[SPEC_PERIODIC + j * SPEC_PERIODIC_STRIDE:][:8]]
            dynamic.append(dict(p1=(p[0], p[1]), p2=(p[2], p[3]), freq=p[4], rx=p[5], ry=p[6], angle=p[7]))
        out.append(dict(boundary=[tuple(map(float, q)) for q in r[SPEC_BOUNDARY:SPEC_BOUNDARY + 2 * nb].reshape(-1, 2)],
                        static=static, dynamic=dynamic, start=[float(x) for x in r[0:5]], goal=[float(x) for x in r[5:7]]))
    return out


def _bind(lib):
    return bind_exports(lib, "map", _MAP_TABLE, "csrc/envgpu.hip, csrc/envimg.hip, csrc/mapgpu.hip")


def draw_specs_dev(spec_table, spare_ready, attempt, seed: int, device: int = 0):
    """Enqueue ``map_draw_kernel`` on the current stream: for every row b with ``spare_ready[b] == 0`` the spec table row
    becomes ``pack_specs([spec_of(seed, b + B * attempt[b])])`` and ``attempt[b]`` grows by one; other rows are left
    alone.  ``spec_table`` float64 [B, SPEC_DOUBLES], ``spare_ready`` and ``attempt`` int32 [B], on the device."""
    import torch
    from .solver import load_library
    lib = _bind(load_library())
    B = spec_table.shape[0]
    if spec_table.shape != (B, SPEC_DOUBLES) or spec_table.dtype != torch.float64 or not spec_table.is_contiguous() or \
            any(t.shape != (B,) or t.dtype != torch.int32 or not t.is_contiguous() for t in (spare_ready, attempt)):
        raise ValueError(f"spec_table must be contiguous float64 [B, {SPEC_DOUBLES}], spare_ready and attempt int32 [B]")
    rc = lib.mpcgpu_map_draw_dev(device, B, C.c_uint64(int(seed) % 2 ** 64), spec_table.data_ptr(), spare_ready.data_ptr(),
                                 attempt.data_ptr(), torch.cuda.current_stream(spec_table.device).cuda_stream)
    if rc != 0:
        raise MpcGpuError(lib.mpcgpu_map_last_error().decode())


def rings_dev(spec_table, spare_ready, device: int = 0, out=None):
    """Enqueue ``map_rings_kernel`` on the current stream: spec table -> (ring records float64 [B, R], start_goal float64
    [B, 4]) as ``path_plan.PathPlanner.plan_dev`` takes them with ``n_vert_max=VERT_MAX, n_ring_max=RING_MAX`` -- bit for
    bit ``pack_rings(oriented_rings(*inflate_spec(spec)))``.  Rows with ``spare_ready != 0`` get ring count 0 (planner
    status 4).  The device code does not repeat the host's validity tests of the offset rings (``include/mpcgpu_map.h``).
    ``out=(rings, start_goal)`` writes into tensors of an earlier call instead of new ones."""
    import torch
    from . import path_plan
    from .solver import load_library
    lib = _bind(load_library())
    B = spec_table.shape[0]
    if spec_table.shape != (B, SPEC_DOUBLES) or spec_table.dtype != torch.float64 or not spec_table.is_contiguous() or \
            spare_ready.shape != (B,) or spare_ready.dtype != torch.int32 or not spare_ready.is_contiguous():
        raise ValueError(f"spec_table must be contiguous float64 [B, {SPEC_DOUBLES}] and spare_ready int32 [B]")
    if out is None:
        rings = torch.empty(B, path_plan.record_doubles(VERT_MAX, RING_MAX), dtype=torch.float64, device=spec_table.device)
        start_goal = torch.empty(B, 4, dtype=torch.float64, device=spec_table.device)
    else:
        rings, start_goal = out
    rc = lib.mpcgpu_map_rings_dev(device, B, spec_table.data_ptr(), spare_ready.data_ptr(), rings.data_ptr(),
                                  start_goal.data_ptr(), torch.cuda.current_stream(spec_table.device).cuda_stream)
    if rc != 0:
        raise MpcGpuError(lib.mpcgpu_map_last_error().decode())
    return rings, start_goal


def records_dev(params, spec_table, plan_status, plan_n_nodes, plan_nodes, records2, which, spare_ready, status, device: int = 0):
    """Enqueue ``map_record_kernel`` on the current stream: for rows with ``spare_ready == 0`` and planner status 0 whose map
    fits ``params`` (``rl_env._CParams`` of the record table) the spare record ``records2[1 - which[b], b]`` becomes what
    ``pack_records([make_map(path=nodes, **spec)], limits=...)`` writes and ``spare_ready[b] = 1``; ``status`` int32 [B]
    receives :data:`STATUS`.  Nothing of a row is written unless its status is 0."""
    import torch
    from .solver import load_library
    lib = _bind(load_library())
    B = spec_table.shape[0]
    rc = lib.mpcgpu_map_record_dev(device, C.byref(params), B, spec_table.data_ptr(), plan_status.data_ptr(),
                                   plan_n_nodes.data_ptr(), plan_nodes.data_ptr(), records2.data_ptr(), which.data_ptr(),
                                   spare_ready.data_ptr(), status.data_ptr(),
                                   torch.cuda.current_stream(spec_table.device).cuda_stream)
    if rc != 0:
        raise MpcGpuError(lib.mpcgpu_map_last_error().decode())
