"""Host-side tests of the device fleet tick (no GPU): the exports of ``include/mpcgpu_fleet.h``, the group table of
``fleet.pack_groups`` and ``fleet.share_numpy`` -- the host twin of ``fleet_share_kernel`` -- against
``BatchedTracker.share_predictions``."""
import ctypes
import importlib
import os
import re
import types

import numpy as np
import pytest

from conftest import make_cfg
from support.fleet_cases import limit_groups, other_groups
from trajtrack_mpcndqn_rlboost_amd import fleet, map_stream, path_plan, per_tree, rl_env
from trajtrack_mpcndqn_rlboost_amd.batched_tracker import BatchedTracker

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")  # (the package attribute `solver` is the plugin factory)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fleet_header_declares_the_exports_and_the_library_has_them():
    text = open(os.path.join(ROOT, "include", "mpcgpu_fleet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mpcgpu_[a-z_0-9]+)\s*\(", text))
    assert declared == set(fleet.FLEET_EXPORTS)
    path = solver_mod.library_path()
    assert os.path.exists(path), f"{path} missing -- run __graft_entry__.build()"
    lib = ctypes.CDLL(path)
    for sym in fleet.FLEET_EXPORTS:
        assert hasattr(lib, sym), sym
    lib.mpcgpu_abi_version.restype = ctypes.c_int32
    assert lib.mpcgpu_abi_version() == 8
    others = set(solver_mod.EXPORTS) | set(rl_env.ENV_EXPORTS) | set(per_tree.PER_EXPORTS) | set(path_plan.PLAN_EXPORTS) | \
        set(map_stream.MAP_EXPORTS)
    assert not set(fleet.FLEET_EXPORTS) & others
    # the solver's header keeps to its own exports
    main_header = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    assert not any(sym + "(" in main_header for sym in fleet.FLEET_EXPORTS)


def test_pack_groups_table_and_colours():
    groups = [[4, 1], [], [0], [5, 2, 3]]
    t = fleet.pack_groups(groups, 6)
    assert t.members.tolist() == [4, 1, 0, 5, 2, 3] and t.members.dtype == np.int32
    assert t.group_start.tolist() == [2, 0, 3, 3, 0, 3]
    assert t.group_len.tolist() == [1, 2, 3, 3, 2, 3]
    assert t.pos.tolist() == [0, 1, 1, 2, 0, 0]
    assert [c.tolist() for c in t.colours] == [[4, 0, 5], [1, 2], [3]]       # the empty group has no colour, the order is the groups'
    assert np.array_equal(t.members[t.group_start + t.pos], np.arange(6))
    one = fleet.pack_groups(None, 3)                                          # default: one group of all robots
    assert one.members.tolist() == [0, 1, 2] and one.group_len.tolist() == [3, 3, 3] and len(one.colours) == 3
    assert fleet.pack_groups([], 0).members.shape == (0,)


@pytest.mark.parametrize("groups", [[[0, 1], [1, 2]], [[0, 1]], [[0, 1, 2, 3]], [[0, 1], [2, -1]], []])
def test_pack_groups_refuses_what_is_not_a_partition(groups):
    """Overlap, a missing robot, a robot out of range."""
    with pytest.raises(ValueError, match=r"groups must partition the robots 0\.\.B-1"):
        fleet.pack_groups(groups, 3)


def test_check_rows_refuses_repeated_and_out_of_range_rows():
    assert fleet.check_rows([3, 0, 2], 4).tolist() == [3, 0, 2] and fleet.check_rows([], 4).dtype == np.int32
    for bad in ([0, 0], [4], [-1], [1, 2, 1]):
        with pytest.raises(ValueError):
            fleet.check_rows(bad, 4)


@pytest.mark.parametrize("N", [20, 40])
def test_share_numpy_equals_the_host_trackers_share_predictions(N):
    cfg = make_cfg(N)
    B, Nother = 40, cfg.Nother
    rng = np.random.default_rng(N)
    # share_predictions never touches the solver: a stub stands in for it, so the host tracker exists without a device
    stub = BatchedTracker(cfg, B, solver=types.SimpleNamespace())
    stub.pred_states[:] = rng.normal(size=(B, N, cfg.ns))
    lim = limit_groups(B, Nother)
    assert sorted(len(g) for g in lim)[:5] == [0, 1, 2, Nother + 1, Nother + 3]
    for groups in (lim, other_groups(B), None, [[i] for i in range(B)]):
        stub.other_robot_states[:] = rng.normal(size=stub.other_robot_states.shape)      # stale content must not survive
        stub.share_predictions(groups)
        got = fleet.share_numpy(fleet.pack_groups(groups, B), stub.pred_states, Nother)
        assert np.array_equal(got, stub.other_robot_states)
    # the truncated group, spelt out: position 12 sees members 0..9, position 0 members 1..10
    big = lim[4]
    assert len(big) == Nother + 3 == 13
    stub.share_predictions(lim)
    blocks = stub.other_robot_states.reshape(B, Nother, N * cfg.ns)
    flat = stub.pred_states.reshape(B, -1)
    assert np.array_equal(blocks[big[12]], flat[big[0:10]]) and np.array_equal(blocks[big[0]], flat[big[1:11]])
    assert np.array_equal(fleet.share_numpy(fleet.pack_groups(lim, B), stub.pred_states, Nother).reshape(blocks.shape), blocks)
