"""TEST INFRASTRUCTURE -- an independent check of the planner twin (tests/support/plan_numpy.py).

Nothing here shares code or method with the twin:

* graph nodes are start, goal and EVERY ring vertex (not only the reflex ones; a vertex buried in another obstacle simply
  sees nothing);
* visibility of p q: the parameters at which p q meets the line of any outline edge (the segment/edge intersection
  parameters of ``oracle/rl_env_numpy.py``'s ray test, solved for both parameters) plus the projections of vertices that lie
  on p q cut the segment into pieces; the MIDPOINT of every piece longer than ``TOL`` must lie in free space, decided by
  ``oracle.rl_env_numpy.winding_number`` (obstacles) and ``rl_geometry.point_in_ring`` (boundary, even-odd).  A midpoint
  closer than ``TOL`` to an outline is ON it (running along an edge) and allowed;
* shortest paths for all pairs by Floyd-Warshall.

So it decides grazing contacts by a distance tolerance where the twin decides them by exact signs: the two may differ on a
contact that is within ``TOL`` of collinear but not exactly so -- in path length only to second order in that distance.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from oracle import rl_env_numpy as orc
from trajtrack_mpcndqn_rlboost_amd import rl_geometry as rg

TOL = 1e-7          # metres: shorter pieces / nearer outlines count as touching


def _outline_distance(pt, ring: np.ndarray) -> float:
    return min(orc.point_segment_distance(pt, ring[i], ring[(i + 1) % len(ring)]) for i in range(len(ring)))


def point_is_free(pt, rings: Sequence[np.ndarray]) -> bool:
    """Closed free space: inside or on ring 0, not strictly inside rings 1.."""
    for k, ring in enumerate(rings):
        if _outline_distance(pt, ring) <= TOL:
            continue
        if k == 0:
            if not rg.point_in_ring(pt, ring):
                return False
        elif orc.winding_number(pt, ring) != 0:
            return False
    return True


def segment_is_free(p, q, rings: Sequence[np.ndarray]) -> bool:
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    d = q - p
    L = math.hypot(d[0], d[1])
    if L <= TOL:
        return point_is_free(p, rings)
    ts = [0.0, 1.0]
    for ring in rings:
        a = np.asarray(ring, dtype=np.float64)
        b = np.roll(a, -1, axis=0)
        e = b - a
        den = d[0] * e[:, 1] - d[1] * e[:, 0]
        ap = a - p
        ok = np.abs(den) > 1e-300
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (ap[:, 0] * e[:, 1] - ap[:, 1] * e[:, 0]) / den
            u = (ap[:, 0] * d[1] - ap[:, 1] * d[0]) / den
        hit = ok & (t > 0.0) & (t < 1.0) & (u >= -1e-9) & (u <= 1.0 + 1e-9)
        ts += t[hit].tolist()
        # vertices on the segment's line (collinear edges have no single crossing)
        tv = (ap[:, 0] * d[0] + ap[:, 1] * d[1]) / (L * L)
        off = np.abs(ap[:, 0] * d[1] - ap[:, 1] * d[0]) / L
        ts += tv[(off <= TOL) & (tv > 0.0) & (tv < 1.0)].tolist()
    ts.sort()
    for t0, t1 in zip(ts[:-1], ts[1:]):
        if (t1 - t0) * L <= TOL:
            continue
        if not point_is_free(p + 0.5 * (t0 + t1) * d, rings):
            return False
    return True


def shortest_length(rings: Sequence[np.ndarray], start, goal) -> float:
    """Length of the shortest start-goal path over ALL ring vertices; inf if there is none; nan if start or goal is not free."""
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]
    if not (point_is_free(start, rings) and point_is_free(goal, rings)):
        return math.nan
    pts = np.concatenate([np.asarray([start[:2], goal[:2]], dtype=np.float64)] + rings)
    n = len(pts)
    D = np.full((n, n), np.inf)
    np.fill_diagonal(D, 0.0)
    for i in range(n):
        for j in range(i + 1, n):
            if segment_is_free(pts[i], pts[j], rings):
                D[i, j] = D[j, i] = math.hypot(pts[j, 0] - pts[i, 0], pts[j, 1] - pts[i, 1])
    for k in range(n):
        D = np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
    return float(D[0, 1])


def near_collinear_triples(rings: Sequence[np.ndarray], start, goal, tol: float = 1e-9) -> int:
    """Triples (node, node, ring vertex strictly between them) within ``tol`` (sine of the angle) of collinear.  Nodes:
    start, goal and all ring vertices."""
    verts = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings])
    pts = np.concatenate([np.asarray([start[:2], goal[:2]], dtype=np.float64), verts])
    count = 0
    for i in range(len(pts)):
        d = pts[i + 1:] - pts[i]                                   # [m, 2]
        w = verts - pts[i]                                         # [v, 2]
        cr = d[:, None, 0] * w[None, :, 1] - d[:, None, 1] * w[None, :, 0]
        dl, wl = np.hypot(d[:, 0], d[:, 1]), np.hypot(w[:, 0], w[:, 1])
        t = d[:, None, 0] * w[None, :, 0] + d[:, None, 1] * w[None, :, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            sine = np.abs(cr) / (dl[:, None] * wl[None, :])
        between = (t > 0.0) & (t < (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None])     # the same expression as t at v == q
        count += int(np.sum(between & (sine < tol)))
    return count
