"""TEST INFRASTRUCTURE -- which branches of the planner's contact rule does a set of maps reach?

``visible`` restates ``plan_numpy.visible`` line by line with a counter on every branch that only an exact contact takes,
``count_map`` adds the contacts that are decided before the graph exists (start or goal on an outline, straight vertices,
covered vertices).  ``counting_twin`` hangs the counters on the twin itself: every call the twin makes is answered by the
twin's own ``visible`` and counted by the restatement, and the two answers must be equal.
"""
from __future__ import annotations

import collections
import contextlib

from . import plan_numpy as twin

START_ON_OUTLINE = "start on an outline"
GOAL_ON_OUTLINE = "goal on an outline"
STRAIGHT_VERTEX = "turn == 0 vertex"
CONE_OF_STRAIGHT_VERTEX = "into_forbidden with t == 0"
COLLINEAR_BLOCKS = "collinear interior vertex that blocks"
COLLINEAR_PASSES = "collinear interior vertex that passes"
P_IN_EDGE_BLOCKS = "op == 0 edge-interior block"
Q_IN_EDGE_BLOCKS = "oq == 0 edge-interior block"
REFLEX_COVERED = "reflex vertex dropped because another ring covers it"
VERTEX_ON_OTHER_OUTLINE = "vertex on another ring's outline"
BRANCHES = (START_ON_OUTLINE, GOAL_ON_OUTLINE, STRAIGHT_VERTEX, CONE_OF_STRAIGHT_VERTEX, COLLINEAR_BLOCKS, COLLINEAR_PASSES,
            P_IN_EDGE_BLOCKS, Q_IN_EDGE_BLOCKS, REFLEX_COVERED, VERTEX_ON_OTHER_OUTLINE)


def into_forbidden(ax, ay, vx, vy, bx, by, dx, dy, C):
    e0x, e0y, e1x, e1y = vx - ax, vy - ay, bx - vx, by - vy
    t = e0x * e1y - e0y * e1x
    c0 = e0x * dy - e0y * dx
    c1 = e1x * dy - e1y * dx
    if t == 0.0:
        C[CONE_OF_STRAIGHT_VERTEX] += 1
    if t > 0.0:
        return c0 < 0.0 or c1 < 0.0
    return c0 < 0.0 and c1 < 0.0


def visible(px, py, qx, qy, X, Y, PREV, NEXT, C):
    dx, dy = qx - px, qy - py
    len2 = dx * dx + dy * dy
    for i in range(len(X)):
        vx, vy = X[i], Y[i]
        ax, ay, bx, by = X[PREV[i]], Y[PREV[i]], X[NEXT[i]], Y[NEXT[i]]
        si = twin.orient2d(px, py, qx, qy, vx, vy)
        if vx == px and vy == py:
            if into_forbidden(ax, ay, vx, vy, bx, by, dx, dy, C):
                return False
        elif vx == qx and vy == qy:
            if into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy, C):
                return False
        elif si == 0.0:
            t = (vx - px) * dx + (vy - py) * dy
            if 0.0 < t < len2:
                if into_forbidden(ax, ay, vx, vy, bx, by, dx, dy, C) or into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy, C):
                    C[COLLINEAR_BLOCKS] += 1
                    return False
                C[COLLINEAR_PASSES] += 1
        sj = twin.orient2d(px, py, qx, qy, bx, by)
        op = twin.orient2d(vx, vy, bx, by, px, py)
        oq = twin.orient2d(vx, vy, bx, by, qx, qy)
        if ((si > 0.0 and sj < 0.0) or (si < 0.0 and sj > 0.0)) and ((op > 0.0 and oq < 0.0) or (op < 0.0 and oq > 0.0)):
            return False
        ex, ey = bx - vx, by - vy
        e2 = ex * ex + ey * ey
        if op == 0.0 and oq < 0.0:
            u = (px - vx) * ex + (py - vy) * ey
            if 0.0 < u < e2:
                C[P_IN_EDGE_BLOCKS] += 1
                return False
        if oq == 0.0 and op < 0.0:
            u = (qx - vx) * ex + (qy - vy) * ey
            if 0.0 < u < e2:
                C[Q_IN_EDGE_BLOCKS] += 1
                return False
    return True


def count_table(rings, start, goal, C):
    """The contacts that are decided before the graph exists."""
    X, Y, PREV, NEXT, RING, spans = twin.ring_table(rings)
    for name, p in ((START_ON_OUTLINE, start), (GOAL_ON_OUTLINE, goal)):
        C[name] += sum(twin.locate(float(p[0]), float(p[1]), X, Y, lo, hi) == 1 for lo, hi in spans)
    for i in range(len(X)):
        a, b = PREV[i], NEXT[i]
        turn = (X[i] - X[a]) * (Y[b] - Y[i]) - (Y[i] - Y[a]) * (X[b] - X[i])
        where = [twin.locate(X[i], Y[i], X, Y, lo, hi) if k != RING[i] else -1 for k, (lo, hi) in enumerate(spans)]
        C[STRAIGHT_VERTEX] += turn == 0.0
        C[REFLEX_COVERED] += turn < 0.0 and 2 in where[1:]
        C[VERTEX_ON_OTHER_OUTLINE] += where.count(1)


def count_map(rings, start, goal, C):
    """``count_table``, then every pair of graph nodes i < j as the kernel evaluates them (unless start or goal is not free)."""
    count_table(rings, start, goal, C)
    X, Y, PREV, NEXT, RING, spans = twin.ring_table(rings)
    sx, sy, gx, gy = float(start[0]), float(start[1]), float(goal[0]), float(goal[1])
    if not (twin.in_free_space(sx, sy, X, Y, spans) and twin.in_free_space(gx, gy, X, Y, spans)):
        return
    cand = twin.candidate_vertices(X, Y, PREV, NEXT, RING, spans)
    nx, ny = [sx, gx] + [X[v] for v in cand], [sy, gy] + [Y[v] for v in cand]
    for i in range(len(nx)):
        for j in range(i + 1, len(nx)):
            assert visible(nx[i], ny[i], nx[j], ny[j], X, Y, PREV, NEXT, C) == twin.visible(nx[i], ny[i], nx[j], ny[j], X, Y, PREV, NEXT)


@contextlib.contextmanager
def counting_twin(C):
    """Inside, ``twin.plan`` counts the branches of the pairs its search asks for into ``C``."""
    real = twin.visible

    def counted(*args):
        answer = real(*args)
        assert visible(*args, C) == answer
        return answer

    twin.visible = counted
    try:
        yield
    finally:
        twin.visible = real


def new_counter():
    return collections.Counter({name: 0 for name in BRANCHES})
