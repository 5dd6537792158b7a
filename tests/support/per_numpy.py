"""Numpy twin of csrc/pergpu.hip (include/mpcgpu_per.h), operation by operation in float64.

What it keeps of the reference's ``PerReplayBuffer`` and what it changes on purpose:

* heap-ordered tree of ``2 C - 1`` doubles, leaf of ring position ``p`` = node ``p + C - 1``;
* an inner node is ALWAYS ``tree[left] + tree[right]``, recomputed depth by depth (deepest first) after a leaf below it
  changed -- the reference adds ``change`` to every ancestor and lets the sums drift;
* ``max_p`` is re-read at most once per ``add`` call, at its start;
* on a repeated index of ``update`` the highest row wins (the reference applies the rows in order: the same);
* the descent never enters a child whose sum is 0: it takes the sibling (the reference retries after a rebuild).

Powers go through ``math.pow`` (the C library's, one scalar at a time), as the reference's scalar ``**`` does.
"""
from __future__ import annotations

import math

import numpy as np


def depth_of(i):
    """floor(log2(i + 1)): the depth of node ``i`` (exact integer arithmetic, scalars or arrays)."""
    v = np.asarray(i, dtype=np.int64) + 1
    d = np.zeros(v.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (v >> s) > 0
        d = np.where(big, d + s, d)
        v = np.where(big, v >> s, v)
    return d


class SumTree:
    def __init__(self, capacity, alpha=0.3, beta=0.4, epsilon=1e-3, update_max_freq=1000, initial_priority=1.0):
        self.C = int(capacity)
        assert self.C >= 1 and update_max_freq >= 1
        self.alpha, self.beta, self.epsilon = float(alpha), float(beta), float(epsilon)
        self.update_max_freq, self.initial_priority = int(update_max_freq), float(initial_priority)
        self.tree = np.zeros(2 * self.C - 1, dtype=np.float64)
        self.D = int(depth_of(2 * self.C - 2))
        self.max_p, self.since = self.initial_priority, float(self.update_max_freq)

    @property
    def leaves(self):
        return self.tree[self.C - 1:]

    def state(self):
        """The head of the device state block: max_p, rows since the last reading, two reserved zeros."""
        return np.array([self.max_p, self.since, 0.0, 0.0])

    def _recompute_ancestors(self, idx):
        idx = np.unique(np.asarray(idx, dtype=np.int64))
        dl = depth_of(idx)
        for d in range(self.D - 1, -1, -1):
            below = dl > d
            nodes = np.unique(((idx[below] + 1) >> (dl[below] - d)) - 1)
            self.tree[nodes] = self.tree[2 * nodes + 1] + self.tree[2 * nodes + 2]

    def add(self, pos, n, n_entries):
        if self.since >= self.update_max_freq:
            self.max_p = float(np.max(self.leaves)) if n_entries > 0 else self.initial_priority
            self.since = 0.0
        self.since += float(n)
        rows = min(int(n), self.C)
        idx = (int(pos) + np.arange(rows, dtype=np.int64)) % self.C + self.C - 1
        self.tree[idx] = self.max_p
        self._recompute_ancestors(idx)

    def priorities(self, td_error):
        """(|td| + epsilon)^alpha in float64, one ``math.pow`` per row."""
        return np.array([math.pow(abs(float(t)) + self.epsilon, self.alpha) for t in np.asarray(td_error, dtype=np.float32)])

    def set_leaves(self, indices, values):
        """Leaf ``indices[r]`` takes ``values[r]`` in row order (the last row of a repeated index wins; a row whose index
        is not a leaf is ignored), then the ancestors are recomputed."""
        indices = np.asarray(indices, dtype=np.int64)
        ok = (indices >= self.C - 1) & (indices <= 2 * self.C - 2)
        for i, v in zip(indices[ok], np.asarray(values, dtype=np.float64)[ok]):
            self.tree[i] = v
        self._recompute_ancestors(indices[ok])

    def update(self, indices, td_error):
        self.set_leaves(indices, self.priorities(td_error))

    def sample(self, u, n_entries):
        """-> (tree indices int64, ring positions int64, weights float64 normalised by their maximum)."""
        u = np.asarray(u, dtype=np.float64)
        n, tree, size = len(u), self.tree, len(self.tree)
        total = tree[0]
        segment = total / np.float64(n)
        indices = np.zeros(n, dtype=np.int64)
        for i in range(n):
            a, b = segment * np.float64(i), segment * np.float64(i + 1)
            s = a + (b - a) * u[i]
            idx, left = 0, 1
            while left < size:
                tl, tr = tree[left], tree[left + 1]
                go_left = s <= tl
                if go_left and tl == 0.0:
                    go_left = False
                elif not go_left and tr == 0.0:
                    go_left = True
                if go_left:
                    idx = left
                else:
                    s = s - tl
                    idx = left + 1
                left = 2 * idx + 1
            indices[i] = idx
        x = np.float64(n_entries) * tree[indices] / total
        w = np.array([math.pow(float(v), -self.beta) for v in x])
        return indices, indices - (self.C - 1), w / np.max(w)


def check_invariant(tree):
    """Every inner node equals the sum of its children, exactly."""
    tree = np.asarray(tree)
    C = (len(tree) + 1) // 2
    inner = np.arange(C - 1)
    return bool(np.array_equal(tree[inner], tree[2 * inner + 1] + tree[2 * inner + 2]))
