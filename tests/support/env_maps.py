"""TEST INFRASTRUCTURE -- seeded random maps for the environment kernels (csrc/envgpu.hip, csrc/envimg.hip).

:func:`random_map` draws a hall with random obstacles on general key-frame animations.  With its default knobs it makes
exactly the draws of the generator that ``tests/test_gpu_env.py`` has always used (tests/test_env_maps.py pins that).
The knobs reach what the fixture scenes do not:

* ``n_obst``: a ``(lo, hi)`` range of obstacle *attempts* (rejected shapes are skipped, as before), or an int: exactly
  that many obstacles (up to 31, the kernels' limit);
* ``n_vert``: ``(lo, hi)`` range of outline vertices per obstacle before padding;
* ``n_kf``: ``(lo, hi)`` range of key frames (1..4); ``interp``: ``"linear"`` / ``"cosine"`` for every obstacle, or
  ``None`` for a random one each; ``offset``: ``(lo, hi)`` of the time offset;
* ``concave``: probability of a star-shaped (concave) obstacle, kept wherever ``rl_geometry.buffer_polygon`` accepts
  its padded outline;
* ``boundary_vertices``: the hall's lower wall as a gentle wave of that many vertices (at most 4 per metre);
* ``n_edge``: pad the boundary ring with points on its own edges until the map has exactly this many outline edges
  (``rl_env.pack_records`` counts one edge per outline vertex).

All ranges are half-open, as ``numpy.random.Generator.integers``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import numpy as np

from trajtrack_mpcndqn_rlboost_amd import rl_geometry as rg

MAX_OBST = 31
MAX_KF = 4


def n_edges(m) -> int:
    """Outline edges of a map as ``rl_env.pack_records`` counts them."""
    return len(m["boundary_padded"]) + sum(len(o["padded_nodes"]) for o in m["obstacles"])


def _pad_to_edges(ring: np.ndarray, total: int) -> np.ndarray:
    """Insert midpoints into the longest edges of ``ring`` until it has ``total`` vertices (the outline is unchanged)."""
    ring = [np.asarray(p, dtype=np.float64) for p in ring]
    while len(ring) < total:
        n = len(ring)
        k = max(range(n), key=lambda i: float(np.hypot(*(ring[(i + 1) % n] - ring[i]))))
        ring.insert(k + 1, 0.5 * (ring[k] + ring[(k + 1) % n]))
    return np.asarray(ring)


def _obstacle(rng, W, H, n_vert, n_kf, interp, offset, concave):
    """One obstacle, or None when the drawn shape is rejected (the draws up to the rejection are made either way)."""
    star = concave > 0.0 and rng.random() < concave
    n = rng.integers(*n_vert)
    if star:
        ang = np.linspace(0, 2 * math.pi, 2 * n, endpoint=False) + rng.uniform(0, math.pi / n)
    else:
        ang = np.sort(rng.uniform(0, 2 * math.pi, n))
        if np.min(np.diff(np.concatenate([ang, [ang[0] + 2 * math.pi]]))) < 0.4:
            return None
    rad = rng.uniform(0.5, 2.0)
    if star:
        rad = np.where(np.arange(2 * n) % 2 == 0, rad + 0.5, (rad + 0.5) * rng.uniform(0.4, 0.7))
    nodes = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    if rg.signed_area(nodes) < 0.3:
        return None
    try:
        padded = rg.buffer_polygon(nodes, 0.5)
    except ValueError:
        return None
    nk = int(rng.integers(*n_kf))
    frames = [(rng.uniform(1, W - 1), rng.uniform(1, H - 1), rng.uniform(-3, 3)) for _ in range(nk)]
    steps = [0.0] + [float(rng.uniform(0.5, 6.0)) for _ in range(nk)]
    kind = "cosine" if rng.random() < 0.5 else "linear"
    return dict(padded_nodes=padded, time_steps=steps, keyframes=frames, interp=interp or kind,
                offset=float(rng.uniform(*offset)))


def random_map(rng, n_obst: Union[int, Tuple[int, int]] = (0, 7), n_vert: Tuple[int, int] = (3, 7),
               n_kf: Tuple[int, int] = (1, MAX_KF + 1), interp: Optional[str] = None,
               offset: Tuple[float, float] = (0.0, 5.0), concave: float = 0.0, boundary_vertices: int = 0,
               n_edge: Optional[int] = None):
    """A random hall with random obstacles on general key-frame animations (1..4 key frames, linear or cosine easing,
    time offsets); the knobs are described in the module docstring."""
    assert interp in (None, "linear", "cosine") and 1 <= n_kf[0] and n_kf[1] <= MAX_KF + 1
    W, H = rng.uniform(12, 30), rng.uniform(10, 25)
    boundary = [(0, 0), (W, 0), (W, H), (0, H)]
    if rng.random() < 0.5:                      # notch: a reflex corner in the boundary
        boundary = [(0, 0), (W, 0), (W, H * 0.6), (W * 0.7, H * 0.6), (W * 0.7, H), (0, H)]
    if boundary_vertices > 0:                   # the lower wall as a wave: many short edges at varied slopes
        # at most 4 vertices per metre, and the wall rises from both corners: buffer_polygon's local construction
        # applies (the rest of an n_edge target is made up by points on the padded ring's edges)
        xs = np.linspace(0.0, W, min(boundary_vertices, int(4 * W)) + 2)[1:-1]
        amp, half_waves = rng.uniform(0.1, 0.25), 2 * int(rng.integers(1, 3)) + 1
        boundary = [(0, 0)] + [(float(x), amp * math.sin(half_waves * math.pi * x / W)) for x in xs] + boundary[1:]
    obstacles = []
    if isinstance(n_obst, (int, np.integer)):
        assert 0 <= n_obst <= MAX_OBST
        while len(obstacles) < n_obst:
            ob = _obstacle(rng, W, H, n_vert, n_kf, interp, offset, concave)
            if ob is not None:
                obstacles.append(ob)
    else:
        for _ in range(rng.integers(*n_obst)):
            ob = _obstacle(rng, W, H, n_vert, n_kf, interp, offset, concave)
            if ob is not None:
                obstacles.append(ob)
    npath = int(rng.integers(2, 9))
    path = np.stack([np.sort(rng.uniform(0.5, W - 0.5, npath)), rng.uniform(0.5, H * 0.55, npath)], axis=1)
    m = dict(start=np.array([path[0, 0], path[0, 1], 0.0, 0.0, 0.0]), goal=np.asarray(path[-1], dtype=np.float32).astype(float),
             path=path, boundary_padded=rg.buffer_polygon(boundary, -0.5), obstacles=obstacles)
    if n_edge is not None:
        have = n_edges(m)
        if have > n_edge:
            raise ValueError(f"the drawn map already has {have} > {n_edge} outline edges")
        m["boundary_padded"] = _pad_to_edges(m["boundary_padded"], len(m["boundary_padded"]) + n_edge - have)
        assert n_edges(m) == n_edge
    return m
