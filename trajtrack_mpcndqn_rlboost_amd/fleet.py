"""Fleet coupling of the device tracker: host side of ``include/mpcgpu_fleet.h`` ("Fleet tick on the device").

A fleet is B robots in groups (the robots of one world, in the reference's dictionary order).  ``pack_groups`` turns the
groups into the robot-indexed table ``fleet_share_kernel`` reads and into the per-colour row lists of a Gauss-Seidel tick
(colour c = the c-th robot of every group that has one); ``share_numpy`` is the kernel's host twin --
``BatchedTracker.share_predictions`` written from the table instead of from the groups.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .solver import CTracker, bind_exports

_VP, _I32 = C.c_void_p, C.c_int32
# export -> (restype, argtypes); include/mpcgpu_fleet.h
_FLEET_TABLE = {
    "mpcgpu_fleet_share_dev": (_I32, [_VP, _I32, _I32] + [_VP] * 6 + [_VP]),
    "mpcgpu_tracker_step_rows_dev": (_I32, [_VP, C.POINTER(CTracker), _VP, _I32, _I32, _VP] + [_VP] * 8 + [_VP]),
}
FLEET_EXPORTS = tuple(_FLEET_TABLE)


class GroupTable(NamedTuple):
    members: np.ndarray       # [B] int32: the groups concatenated, each in its own order
    group_start: np.ndarray   # [B] int32: robot -> where its group begins in ``members``
    group_len: np.ndarray     # [B] int32: robot -> robots in its group
    pos: np.ndarray           # [B] int32: robot -> its position inside its group
    colours: List[np.ndarray]  # colour c -> int32 robots at position c of every group that has one, in group order


def pack_groups(groups: Optional[Sequence[Sequence[int]]], B: int) -> GroupTable:
    """The group table of ``B`` robots.  ``None`` = one group of all robots.  Empty groups are allowed and skipped; anything
    that is not a partition of 0..B-1 raises ``ValueError`` (the message of ``BatchedTracker.step``)."""
    B = int(B)
    if groups is None:
        groups = [list(range(B))]
    lists = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    covered = np.sort(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.int64)
    if not np.array_equal(covered, np.arange(B)):
        raise ValueError("groups must partition the robots 0..B-1")
    lists = [g for g in lists if len(g)]
    members = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32)
    group_start, group_len, pos = (np.zeros(B, dtype=np.int32) for _ in range(3))
    at = 0
    for g in lists:
        group_start[g], group_len[g], pos[g] = at, len(g), np.arange(len(g))
        at += len(g)
    depth = max((len(g) for g in lists), default=0)
    colours = [np.array([g[c] for g in lists if len(g) > c], dtype=np.int32) for c in range(depth)]
    return GroupTable(members, group_start, group_len, pos, colours)


def share_numpy(table: GroupTable, pred_states: np.ndarray, Nother: int) -> np.ndarray:
    """[B, Nother * N * 3]: what ``fleet_share_kernel`` writes -- slot s of robot b holds the prediction of member
    ``s if s < pos[b] else s + 1`` of b's group, for the first ``min(group_len[b] - 1, Nother)`` slots; zeros elsewhere."""
    pred = np.asarray(pred_states, dtype=np.float64)
    B = pred.shape[0]
    per = int(np.prod(pred.shape[1:]))
    out = np.zeros((B, Nother * per))
    if B == 0 or Nother == 0:
        return out
    s = np.arange(Nother)[None, :]
    keep = np.minimum(table.group_len - 1, Nother)[:, None]
    at = table.group_start[:, None] + np.where(s < table.pos[:, None], s, s + 1)
    src = table.members[np.minimum(at, B - 1)]
    block = np.where((s < keep)[:, :, None], pred.reshape(B, per)[src], 0.0)
    return block.reshape(B, Nother * per)


def check_rows(rows, B: int) -> np.ndarray:
    """int32 copy of a row list; ``ValueError`` unless the rows are distinct robots in 0..B-1 (the device cannot check)."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1)
    if len(r) and (r.min() < 0 or r.max() >= B):
        raise ValueError(f"rows must lie in 0..{B - 1}")
    if len(np.unique(r)) != len(r):
        raise ValueError("rows must be distinct")
    return r.astype(np.int32)


def _bind(lib):
    return bind_exports(lib, "fleet", _FLEET_TABLE, "csrc/trackgpu.hip, csrc/mpcgpu.hip")
