"""TEST INFRASTRUCTURE -- the twin of the visibility-graph planner kernel (csrc/plangpu.hip).

Every function restates its device counterpart operation by operation in float64 scalars (Python floats, no fused
multiply-add, ``math.sqrt`` correctly rounded as the device's ``sqrt``), so status, node count, node coordinates and
length must equal the kernel's bit for bit.  The kernel evaluates every pair of nodes, the twin only the pairs Dijkstra
asks for -- always as (lower node index, higher node index), the order the kernel uses.

Rings: ring 0 the boundary counter-clockwise, the others obstacles clockwise (``path_plan.oriented_rings``), so free space
lies to the LEFT of every directed edge and the forbidden open set (obstacle interior, boundary exterior) to the right.

The contact rule (shared with the kernel).  A segment p q is blocked by a ring iff one of:

1. proper crossing: the end points of an edge lie strictly on both sides of p q AND p, q strictly on both sides of the edge;
2. cone at a ring vertex v with neighbours a, b (``into_forbidden``): a direction d leaves v into the forbidden set iff
   it is strictly right of a->v and/or strictly right of v->b -- "or" at a corner that turns left (free cone < 180 deg),
   "and" otherwise.  Tested with d = q - p where v == p, d = p - q where v == q (coordinates compared), and with both
   d and -d where v lies on the open segment (orient(p, q, v) == 0 and 0 < (v - p).(q - p) < |q - p|^2);
3. touching: p lies on the open edge (orient(a, b, p) == 0, 0 < (p - a).(b - a) < |b - a|^2) and q strictly right of it;
   the same with p and q exchanged.

Everything else -- running along an edge, touching a vertex from the free side -- is allowed.  All signs come from the ONE
expression ``orient2d``; "== 0" means that expression evaluates to zero in float64.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import numpy as np

MAX_VERTICES = 256
MAX_RINGS = 32
MAX_PATH_NODES = 64

OK, NO_PATH, NOT_FREE, TOO_MANY_NODES = 0, 1, 2, 3


def orient2d(ax, ay, bx, by, cx, cy):
    """> 0: c left of a->b."""
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def locate(px, py, X, Y, lo, hi):
    """Point against ring vertices lo .. hi - 1: 0 strictly outside, 1 on the outline, 2 strictly inside (even-odd)."""
    inside = False
    for i in range(lo, hi):
        j = i + 1 if i + 1 < hi else lo
        ax, ay, bx, by = X[i], Y[i], X[j], Y[j]
        o = orient2d(ax, ay, bx, by, px, py)
        if o == 0.0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return 1
        if (ay > py) != (by > py) and (o > 0.0) == (by > ay):
            inside = not inside
    return 2 if inside else 0


def into_forbidden(ax, ay, vx, vy, bx, by, dx, dy):
    e0x, e0y, e1x, e1y = vx - ax, vy - ay, bx - vx, by - vy
    t = e0x * e1y - e0y * e1x
    c0 = e0x * dy - e0y * dx
    c1 = e1x * dy - e1y * dx
    if t > 0.0:
        return c0 < 0.0 or c1 < 0.0
    return c0 < 0.0 and c1 < 0.0


def visible(px, py, qx, qy, X, Y, PREV, NEXT):
    dx, dy = qx - px, qy - py
    len2 = dx * dx + dy * dy
    for i in range(len(X)):
        vx, vy = X[i], Y[i]
        ax, ay, bx, by = X[PREV[i]], Y[PREV[i]], X[NEXT[i]], Y[NEXT[i]]
        si = orient2d(px, py, qx, qy, vx, vy)
        if vx == px and vy == py:
            if into_forbidden(ax, ay, vx, vy, bx, by, dx, dy):
                return False
        elif vx == qx and vy == qy:
            if into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy):
                return False
        elif si == 0.0:
            t = (vx - px) * dx + (vy - py) * dy
            if 0.0 < t < len2 and (into_forbidden(ax, ay, vx, vy, bx, by, dx, dy) or
                                   into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy)):
                return False
        # the edge v -> b
        sj = orient2d(px, py, qx, qy, bx, by)
        op = orient2d(vx, vy, bx, by, px, py)
        oq = orient2d(vx, vy, bx, by, qx, qy)
        if ((si > 0.0 and sj < 0.0) or (si < 0.0 and sj > 0.0)) and ((op > 0.0 and oq < 0.0) or (op < 0.0 and oq > 0.0)):
            return False
        ex, ey = bx - vx, by - vy
        e2 = ex * ex + ey * ey
        if op == 0.0 and oq < 0.0:
            u = (px - vx) * ex + (py - vy) * ey
            if 0.0 < u < e2:
                return False
        if oq == 0.0 and op < 0.0:
            u = (qx - vx) * ex + (qy - vy) * ey
            if 0.0 < u < e2:
                return False
    return True


def ring_table(rings: Sequence[np.ndarray]):
    """(X, Y, PREV, NEXT, ring of each vertex, [(lo, hi)] per ring) in table order."""
    X, Y, PREV, NEXT, RING, spans = [], [], [], [], [], []
    for k, ring in enumerate(rings):
        ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        lo, n = len(X), len(ring)
        for i in range(n):
            X.append(float(ring[i, 0]))
            Y.append(float(ring[i, 1]))
            PREV.append(lo + (i - 1) % n)
            NEXT.append(lo + (i + 1) % n)
            RING.append(k)
        spans.append((lo, lo + n))
    return X, Y, PREV, NEXT, RING, spans


def in_free_space(px, py, X, Y, spans) -> bool:
    if locate(px, py, X, Y, *spans[0]) == 0:
        return False
    return all(locate(px, py, X, Y, lo, hi) != 2 for lo, hi in spans[1:])


def candidate_vertices(X, Y, PREV, NEXT, RING, spans) -> List[int]:
    """Ring vertices that are graph nodes, in table order."""
    out = []
    for i in range(len(X)):
        a, b = PREV[i], NEXT[i]
        turn = (X[i] - X[a]) * (Y[b] - Y[i]) - (Y[i] - Y[a]) * (X[b] - X[i])
        if not turn < 0.0:
            continue
        if RING[i] != 0 and locate(X[i], Y[i], X, Y, *spans[0]) == 0:
            continue
        if any(k != RING[i] and locate(X[i], Y[i], X, Y, *spans[k]) == 2 for k in range(1, len(spans))):
            continue
        out.append(i)
    return out


def plan(rings: Sequence[np.ndarray], start, goal, max_nodes: int = MAX_PATH_NODES) -> Dict:
    """One map -> dict(status, n_nodes, nodes [n_nodes, 2], length)."""
    X, Y, PREV, NEXT, RING, spans = ring_table(rings)
    assert len(X) <= MAX_VERTICES and len(spans) <= MAX_RINGS and max_nodes <= MAX_PATH_NODES
    sx, sy, gx, gy = float(start[0]), float(start[1]), float(goal[0]), float(goal[1])
    none = dict(n_nodes=0, nodes=np.zeros((0, 2)), length=0.0)
    if not (in_free_space(sx, sy, X, Y, spans) and in_free_space(gx, gy, X, Y, spans)):
        return dict(status=NOT_FREE, **none)
    cand = candidate_vertices(X, Y, PREV, NEXT, RING, spans)
    NX = [sx, gx] + [X[i] for i in cand]
    NY = [sy, gy] + [Y[i] for i in cand]
    N = len(NX)
    seen: Dict = {}

    def sees(u, v):
        i, j = (u, v) if u < v else (v, u)
        if (i, j) not in seen:
            seen[(i, j)] = visible(NX[i], NY[i], NX[j], NY[j], X, Y, PREV, NEXT)
        return seen[(i, j)]

    dist, parent, done = [math.inf] * N, [-1] * N, [False] * N
    dist[0] = 0.0
    while True:
        u, best = -1, math.inf
        for k in range(N):
            if not done[k] and dist[k] < best:
                u, best = k, dist[k]
        if u < 0:
            return dict(status=NO_PATH, **none)
        if u == 1:
            break
        done[u] = True
        for v in range(N):
            if done[v] or v == u or not sees(u, v):
                continue
            ddx, ddy = NX[v] - NX[u], NY[v] - NY[u]
            nd = best + math.sqrt(ddx * ddx + ddy * ddy)
            if nd < dist[v]:
                dist[v], parent[v] = nd, u
    back = [1]
    while back[-1] != 0:
        back.append(parent[back[-1]])
    if len(back) > max_nodes:
        return dict(status=TOO_MANY_NODES, n_nodes=len(back), nodes=np.zeros((0, 2)), length=0.0)
    order = back[::-1]
    nodes = np.array([(NX[k], NY[k]) for k in order])
    length = 0.0
    for k in range(len(order) - 1):
        ddx, ddy = nodes[k + 1][0] - nodes[k][0], nodes[k + 1][1] - nodes[k][1]
        length = length + math.sqrt(ddx * ddx + ddy * ddy)
    return dict(status=OK, n_nodes=len(order), nodes=nodes, length=length)


def plan_batch(ring_lists, starts, goals):
    res = [plan(r, s, g) for r, s, g in zip(ring_lists, starts, goals)]
    return (np.array([r["status"] for r in res], dtype=np.int32), np.array([r["n_nodes"] for r in res], dtype=np.int32),
            np.array([r["length"] for r in res]), [r["nodes"] for r in res])
