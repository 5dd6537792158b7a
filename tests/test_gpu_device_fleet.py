"""GPU (-m gpu): fleet coupling ON THE DEVICE TRACKER (include/mpcgpu_fleet.h; csrc/trackgpu.hip fleet_share_kernel, the row-list
forms of tracker_assemble_kernel / tracker_apply_kernel) against the host tracker, whose Gauss-Seidel tick
tests/test_gpu_fleet.py pins bit for bit against the reference's sequential loop.

Same inputs give bitwise the same records and therefore bitwise the same solves; the rollouts behind a solve use the device
library's sin / cos, so taken and predicted states are compared within the bounds of tests/test_gpu_device_tracker.py (1e-12,
1e-11) and the device is put back on the host's state wherever a test compares tick after tick.

The goals lie further away than base_speed * N_hor * ts (4.8 m at N_hor = 20, 9.6 m at 40), so the speed reference is the constant
of the work mode.  Nearer to the goal it is hypot(state - goal) / N / ts, and hypot's last bit differs between libm and the device
library (tests/test_gpu_device_tracker.py compares that block of the record to 1 ulp): the records -- and a solve of hundreds of
PANOC steps behind them -- are then no longer bitwise comparable between host and device assembly.  Robots that stand exactly
on their goal (distance 0 on both sides) are the exception the stop_when_done test uses."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_cfg
from support.fleet_cases import limit_groups, other_groups, world
from trajtrack_mpcndqn_rlboost_amd import BatchSolver, fleet
from trajtrack_mpcndqn_rlboost_amd.batched_tracker import BatchedTracker
from trajtrack_mpcndqn_rlboost_amd.device_tracker import DeviceTracker
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

pytestmark = pytest.mark.gpu

ARRAYS = ("states", "pred_states", "last_actions", "idx_ref", "active", "other", "arrived")


def _fleet(cfg, sizes, solver, n_host=1, n_dev=1):
    """Worlds of ``sizes[w]`` robots on crossing paths: (groups, host trackers, device trackers), all from the same state."""
    B = sum(sizes)
    hosts = [BatchedTracker(cfg, B, solver=solver) for _ in range(n_host)]
    devs = [DeviceTracker(cfg, B, solver=solver) for _ in range(n_dev)]
    groups, i = [], 0
    for w, R in enumerate(sizes):
        starts, goals, paths = world(w, R, x_goal=10.0 if cfg.N_hor <= 20 else 16.0)
        for r in range(R):
            for t in hosts + devs:
                t.initialization(i + r, starts[r].copy(), goals[r], paths[r], "work")
        groups.append(list(range(i, i + R)))
        i += R
    for d in devs:
        d.view()                                                     # uploads the set-up
    return groups, hosts, devs


def _sync(dev, host, idx_ref=True):
    """Put the device tracker on the host tracker's state."""
    dev.states.copy_(torch.from_numpy(host.states))
    dev.pred_states.copy_(torch.from_numpy(host.pred_states))
    dev.last_actions.copy_(torch.from_numpy(host.last_actions))
    if idx_ref:
        dev.idx_ref.copy_(torch.from_numpy(host.idx_ref.astype(np.int32)))


def _np(t):
    return t.cpu().numpy()


# ---- 1. the share kernel at its limits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 40])
def test_share_kernel_equals_the_host_block_at_the_limits_of_the_group_sizes(N):
    cfg = make_cfg(N)
    B, Nother = 40, cfg.Nother
    solver = BatchSolver(cfg)
    host = BatchedTracker(cfg, B, solver=solver)
    dev = DeviceTracker(cfg, B, solver=solver)
    rng = np.random.default_rng(N)
    lim = limit_groups(B, Nother)
    host.pred_states[:] = rng.normal(size=host.pred_states.shape)
    dev.pred_states.copy_(torch.from_numpy(host.pred_states))
    dev.other.copy_(torch.from_numpy(rng.normal(size=(B, dev.other.shape[1]))))      # stale content everywhere
    host.share_predictions(lim)
    dev.share_predictions(lim)
    torch.cuda.synchronize()
    got = _np(dev.other)
    assert np.array_equal(got, host.other_robot_states)
    big = lim[4]                                                   # Nother + 3 robots: truncated
    blocks, flat = got.reshape(B, Nother, -1), host.pred_states.reshape(B, -1)
    assert len(big) == Nother + 3
    assert np.array_equal(blocks[big[12]], flat[big[0:10]]) and np.array_equal(blocks[big[0]], flat[big[1:11]])
    assert not got[lim[0][0]].any() and not got[lim[1][0]].reshape(Nother, -1)[1:].any()      # a lone robot; a pair: one slot
    assert got[lim[3][0]].all()                                    # Nother + 1 robots: exactly full
    # other groups on the same tracker, other predictions: slots of groups that shrank are zero again
    pairs = other_groups(B)
    host.pred_states[:] = rng.normal(size=host.pred_states.shape)
    dev.pred_states.copy_(torch.from_numpy(host.pred_states))
    host.share_predictions(pairs)
    dev.set_groups(pairs)
    dev.share_predictions()
    torch.cuda.synchronize()
    again = _np(dev.other)
    assert np.array_equal(again, host.other_robot_states)
    assert not again.reshape(B, Nother, -1)[:, 1:].any() and got.reshape(B, Nother, -1)[big, 1:].all()
    solver.close()


# ---- 2. Jacobi closed loop ---------------------------------------------------------------------------------------------
def test_jacobi_closed_loop_follows_the_host_tracker():
    cfg = make_cfg(20)
    solver = BatchSolver(cfg)
    groups, (host,), (dev,) = _fleet(cfg, [2, 2, 2], solver)
    coupled = 0
    for tick in range(6):
        _sync(dev, host)
        host.share_predictions(groups)
        a_h, pred_h, cost_h = host.step()
        dev.share_predictions(groups)
        out = dev.step()
        torch.cuda.synchronize()
        assert np.array_equal(_np(dev.other), host.other_robot_states), tick
        assert np.array_equal(_np(out["u"]), host.last_result.solution), tick
        assert np.array_equal(_np(out["cost"]), cost_h) and np.array_equal(_np(out["status"]), host.last_result.status)
        assert np.array_equal(_np(dev.active).astype(bool), host.active)
        assert np.array_equal(_np(dev.idx_ref), host.idx_ref)
        assert np.abs(_np(dev.states) - host.states).max() < 1e-12
        assert np.abs(_np(dev.pred_states) - pred_h).max() < 1e-11
        coupled += int(host.other_robot_states.any())
    assert coupled >= 5                                            # from the second tick on the fleet blocks are in use
    solver.close()


# ---- 3. Gauss-Seidel, colour by colour -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,sizes,T", [(20, [2, 2, 2], 4), (20, [3, 3], 4), (20, [3, 1, 2], 4), (40, [2, 2], 2)])
def test_gauss_seidel_colours_equal_the_host_trackers_pieces(N, sizes, T):
    cfg = make_cfg(N)
    solver = BatchSolver(cfg)
    groups, (host,), (dev,) = _fleet(cfg, sizes, solver)
    dev.set_groups(groups)
    colours = fleet.pack_groups(groups, host.B).colours
    assert len(colours) == max(sizes) and len(colours[-1]) == sum(s == max(sizes) for s in sizes)
    coupled = 0
    for tick in range(T):
        _sync(dev, host)
        refs_h = host.local_refs()
        refs_d = dev.local_refs()
        torch.cuda.synchronize()
        assert np.array_equal(_np(dev.idx_ref), host.idx_ref) and np.array_equal(_np(refs_d), refs_h)
        for c, idx in enumerate(colours):
            idx = idx.astype(np.int64)
            host.share_predictions(groups)
            P = host.assemble("work", refs_h)
            res = solver.solve(P[idx])
            host._apply(idx, res.solution)
            dev.share_predictions()
            # a colour of the uploaded table, or the same rows as a plain list (checked and uploaded by the call)
            out = dev.step_rows(dev.colour_rows[c] if tick % 2 == 0 else idx.tolist())
            torch.cuda.synchronize()
            assert np.array_equal(_np(dev.other), host.other_robot_states), (tick, c)
            assert np.array_equal(_np(out["u"])[idx], res.solution), (tick, c)
            assert np.array_equal(_np(out["cost"])[idx], res.cost) and np.array_equal(_np(out["status"])[idx], res.status)
            assert np.array_equal(_np(out["inner_it"])[idx], res.num_inner_iterations)
            assert np.abs(_np(dev.states) - host.states).max() < 1e-12
            assert np.abs(_np(dev.pred_states) - host.pred_states).max() < 1e-11
            assert np.array_equal(_np(dev.last_actions), host.last_actions)
            _sync(dev, host, idx_ref=False)
        coupled += int(host.other_robot_states.any())
    assert coupled >= T - 1
    solver.close()


# ---- 4. step(groups=...) as one call ---------------------------------------------------------------------------------------
def test_step_with_groups_is_the_sequence_of_share_and_step_rows():
    cfg = make_cfg(20)
    solver = BatchSolver(cfg)
    G, R = 2, 3
    groups, _, (one, seq, jac) = _fleet(cfg, [R] * G, solver, n_host=0, n_dev=3)
    seq.set_groups(groups)
    for tick in range(4):
        out_one = one.step(groups=groups)
        seq.local_refs()
        for c in range(len(seq.colour_rows)):
            seq.share_predictions()
            out_seq = seq.step_rows(seq.colour_rows[c])
        if tick < 3:
            jac.share_predictions(groups)
            out_jac = jac.step()
        torch.cuda.synchronize()
        for name in ARRAYS:
            assert torch.equal(getattr(one, name), getattr(seq, name)), (tick, name)
        for name in out_one:
            assert torch.equal(out_one[name], out_seq[name]), (tick, name)
        assert int((out_one["status"] >= 0).sum()) == G * R and bool(one.other.any()) == (tick > 0 or R > 1)
        if tick == 2:
            # Gauss-Seidel is not Jacobi: after three ticks from the same state the later colours have taken other actions
            later = torch.tensor([g[c] for g in groups for c in range(1, R)], device=one.device)
            assert not torch.equal(out_jac["actions"][later], out_one["actions"][later])
    solver.close()


# ---- 5. the simulator's rule: nobody is frozen -----------------------------------------------------------------------------
def test_stop_when_done_false_reports_arrival_and_keeps_solving():
    cfg = make_cfg(20)
    solver = BatchSolver(cfg)
    groups, (host, host_stop), (dev, dev_stop) = _fleet(cfg, [2, 2], solver, n_host=2, n_dev=2)
    at_goal = [g[0] for g in groups]                               # one robot per world stands on its goal, last action zero
    for h, d in ((host, dev), (host_stop, dev_stop)):
        h.states[at_goal] = h.goals[at_goal]
        _sync(d, h)
    host.stop_when_done = dev.stop_when_done = False
    host.share_predictions(groups)
    a_h, _, cost_h = host.step()
    dev.share_predictions(groups)
    out = dev.step()
    torch.cuda.synchronize()
    assert host.arrived[at_goal].all() and host.arrived.sum() == len(at_goal) and host.active.all()
    assert np.array_equal(_np(dev.arrived).astype(bool), host.arrived)
    assert np.array_equal(_np(dev.active).astype(bool), host.active)
    assert np.array_equal(_np(out["u"]), host.last_result.solution) and np.array_equal(_np(out["cost"]), cost_h)
    assert np.array_equal(_np(out["actions"]), a_h) and _np(out["u"])[at_goal].any(axis=1).all()       # it was solved ...
    assert np.array_equal(_np(dev.last_actions), host.last_actions)
    assert np.abs(_np(dev.states) - host.states).max() < 1e-12                                           # ... and moved like the host's
    # the default: the robot is frozen, its action is 0
    assert dev_stop.stop_when_done and host_stop.stop_when_done
    a_s, _, _ = host_stop.step()
    out_s = dev_stop.step()
    torch.cuda.synchronize()
    assert not host_stop.active[at_goal].any()
    assert np.array_equal(_np(dev_stop.active).astype(bool), host_stop.active)
    assert np.array_equal(_np(out_s["actions"]), a_s) and not _np(out_s["actions"])[at_goal].any()
    assert np.array_equal(_np(dev_stop.states)[at_goal], host_stop.goals[at_goal])
    # a colour with the default rule goes through the row-list kernels: frozen all the same
    dev_stop.active.fill_(1)
    dev_stop.step_rows(at_goal)
    torch.cuda.synchronize()
    assert not _np(dev_stop.active)[at_goal].any() and _np(dev_stop.arrived)[at_goal].all()
    assert not _np(dev_stop.out["actions"])[at_goal].any()
    solver.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_bad_rows_and_groups_are_refused_before_anything_is_enqueued():
    cfg = make_cfg(20)
    solver = BatchSolver(cfg)
    groups, _, (dev,) = _fleet(cfg, [2, 2], solver, n_host=0)
    dev.step(groups=groups)
    torch.cuda.synchronize()
    before = {k: getattr(dev, k).clone() for k in ARRAYS}
    out_before = {k: v.clone() for k, v in dev.out.items()}
    for rows in ([0, 0], [1, 2, 1], [4], [-1, 0], [0, 1, 2, 3, 3]):
        with pytest.raises(ValueError):
            dev.step_rows(rows)
    for bad in ([[0, 1], [1, 2, 3]], [[0, 1], [2]], [[0, 1, 2, 3, 4]], []):
        for call in (dev.set_groups, dev.share_predictions, lambda g: dev.step(groups=g)):
            with pytest.raises(ValueError, match="groups must partition the robots"):
                call(bad)
    # the C entry points: argument errors come back as -1 with a message
    lib, view = fleet._bind(solver._L), dev.view()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in dev.out.items()}
    refs, rows = C.c_void_p(dev.refs.data_ptr()), C.c_void_p(dev.colour_rows[0][0].data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rows_call(rows, n, refs=refs, u=p["u"]):
        return lib.mpcgpu_tracker_step_rows_dev(solver._h, C.byref(view), rows, n, 1, None, refs, None, u, p["cost"], p["status"],
                                                None, None, None, st)
    for rc in (rows_call(rows, -1), rows_call(rows, 5), rows_call(None, 3), rows_call(rows, 2, refs=None), rows_call(rows, 2, u=None)):
        assert rc == -1 and solver._L.mpcgpu_last_error(solver._h)
    tbl = [C.c_void_p(t.data_ptr()) for t in dev._table]
    pred, other = C.c_void_p(dev.pred_states.data_ptr()), C.c_void_p(dev.other.data_ptr())
    assert lib.mpcgpu_fleet_share_dev(solver._h, 4, 40, *tbl, pred, other, st) == -1         # another horizon than the handle's
    assert b"N_hor=20" in solver._L.mpcgpu_last_error(solver._h)
    assert lib.mpcgpu_fleet_share_dev(solver._h, 4, 20, tbl[0], None, tbl[2], tbl[3], pred, other, st) == -1
    assert lib.mpcgpu_fleet_share_dev(solver._h, -1, 20, *tbl, pred, other, st) == -1
    torch.cuda.synchronize()
    for k in ARRAYS:
        assert torch.equal(getattr(dev, k), before[k]), k
    for k, v in dev.out.items():
        assert torch.equal(v, out_before[k]), k
    with pytest.raises(MpcGpuError):
        dev._step_rows((dev.colour_rows[0][0], dev.colour_rows[0][1]), None, None, None)     # refs missing: the library's refusal
    solver.close()
