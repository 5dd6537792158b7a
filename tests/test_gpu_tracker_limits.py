"""GPU (-m gpu): the five small kernels of the device tracker and the hybrid loop (csrc/trackgpu.hip, csrc/mpc_tracker.hpp) at
their limits.  The yardstick is always the numpy host form (BatchedTracker, dqn.rl_reference, hybrid.BatchedHintSwitcher /
tracked_reference), which tests/test_tracker_harness.py and tests/test_hybrid_logic.py pin to the scalar classes of the reference:

* window search with action_steps up to N_hor (66, 120 and 240 candidates: two to four chunks of 64 lanes), exact ties inside a
  chunk, on a chunk boundary and across distant chunks, windows clamped at either end of the reference, references shorter than
  the horizon and than the window, one length per robot;
* the termination test and the speed rule of the assembly kernel exactly on their thresholds;
* the post-solve kernel with action_steps = 3 and 40, robots parked on their goals, no action buffer;
* the proposal rollout for 1 and 40 steps, every action, both clamps, the speed fallback, packed and strided agent rows;
* the switcher kernel with a proposal shorter and longer than the reference, no obstacles, no `live` mask, thresholds hit exactly;
* DeviceHybrid next to BatchedHybrid at N_hor = 40.

Every buffer a kernel writes per robot carries one sentinel row behind robot B - 1 that must come back untouched."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_cfg
from trajtrack_mpcndqn_rlboost_amd.batched_tracker import BatchedTracker
from trajtrack_mpcndqn_rlboost_amd.device_tracker import DeviceTracker
from trajtrack_mpcndqn_rlboost_amd.solver import MpcGpuError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dqn = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn")
hybrid = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.hybrid")
LIMITS = (dqn.ACCELERATION_MAX, dqn.ACCELERATION_MIN, dqn.ANGULAR_ACCELERATION_MAX, dqn.ANGULAR_ACCELERATION_MIN,
          dqn.SPEED_MIN, dqn.SPEED_MAX, dqn.ANGULAR_VELOCITY_MIN, dqn.ANGULAR_VELOCITY_MAX)
NAN = float("nan")


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream      # ordered with the torch copies around the calls


# ---- window search ----------------------------------------------------------------------------------------------------------
WINDOW_CASES = [(20, 1), (20, 11), (20, 20), (40, 40)]     # 6, 66 (second chunk: 2 live lanes), 120 and 240 (four chunks) candidates


def _window_both(solver, N, a, ref, ref_len, idx, xy):
    """One window search of B robots on both sides, everything written directly: ref [B, cap, 3] (NaN behind every robot's own
    length: nothing there may be read), ref_len, idx_ref, xy [B, 2].  Returns the host's (next indices, windows) after asserting
    that the kernel's are bitwise the same and that the row behind robot B - 1 was left alone."""
    B = len(ref_len)
    cfg = make_cfg(N, action_steps=a)
    host = BatchedTracker(cfg, B, solver=solver)
    dev = DeviceTracker(cfg, B, solver=solver)
    dev.view()                                               # nothing pending may overwrite what is written next
    host._ref, host._ref_len, host.idx_ref = np.array(ref), np.asarray(ref_len, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    host.states[:, :2] = xy
    dev.ref = torch.from_numpy(np.ascontiguousarray(ref)).to(_dev())
    dev.ref_len.copy_(torch.from_numpy(np.asarray(ref_len, dtype=np.int32)))
    dev.idx_ref.copy_(torch.from_numpy(np.asarray(idx, dtype=np.int32)))
    dev.states.copy_(torch.from_numpy(host.states))
    out = torch.full((B + 1, N, 3), NAN, dtype=torch.float64, device=_dev())
    solver.tracker_window(dev.view(), out, stream=_stream())
    got, idx_d = out.cpu().numpy(), dev.idx_ref.cpu().numpy()
    want = host.local_refs()
    assert np.isnan(got[B]).all()                            # the sentinel row
    assert np.array_equal(idx_d, host.idx_ref), (idx_d, host.idx_ref)
    assert np.array_equal(got[:B], want)                     # (a NaN read from behind a reference's end would fail here)
    return host.idx_ref.copy(), want


def _run_fleet(solver, N, a, B, ref, ref_len, idx, xy, limit=None):
    """The M robots of a case as one batch of 67 (cycled) or one at a time (B = 1: the first `limit`)."""
    M = len(ref_len)
    if B == 1:
        res = [_window_both(solver, N, a, ref[i:i + 1], ref_len[i:i + 1], idx[i:i + 1], xy[i:i + 1]) for i in range(min(M, limit or M))]
        return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    sel = np.arange(B) % M
    got_idx, got_win = _window_both(solver, N, a, ref[sel], ref_len[sel], idx[sel], xy[sel])
    return got_idx[:M], got_win[:M]


def _pack(rows):
    """rows: list of (ref [len, 3], idx, xy) -> padded table (NaN behind each length), lengths, indices, positions."""
    lens = np.array([len(r[0]) for r in rows])
    ref = np.full((len(rows), lens.max(), 3), NAN)
    for i, r in enumerate(rows):
        ref[i, :lens[i]] = r[0]
    return ref, lens, np.array([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=float)


def _line(n):
    """Straight reference with dyadic spacing: sample k at (k / 4, 0)."""
    return np.stack([0.25 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)


@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("N,a", WINDOW_CASES)
def test_window_search_on_random_references_of_every_length(N, a, B, solver20, solver40):
    solver = solver20 if N == 20 else solver40
    rng = np.random.default_rng(100 * N + a)
    M = 67
    lens = 1 + 4 * rng.permutation(M)                        # 1 .. 265, every robot another one, under one ref_cap
    lens[:8] = [1, N - 3, 60, 6 * a + 30, 6 * a + 30, 6 * a + 30, 5 * a + 2, 2]
    for trial in range(3 if B > 1 else 1):
        rows = []
        for i in range(M):
            n = int(lens[i])
            heading = np.cumsum(rng.normal(0, 0.15, n))
            pts = np.cumsum(0.2 * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0) + rng.uniform(0, 5, 2)
            idx = int(rng.integers(0, n))
            if i in (0, 1, 3, 7):
                idx = 0                                      # lb clamps to 0; len = 1; len < N: the tail repeats the last sample
            elif i == 2:
                idx = min(10, n - 1)                         # 60 samples: ub clamps to len, the other lanes are dead
            elif i in (4, 6):
                idx = n - 1                                  # the last sample
            k = int(np.clip(idx + rng.integers(-a, 6 * a + 1), 0, n - 1))
            rows.append((np.concatenate([pts, heading[:, None]], axis=1), idx, pts[k] + rng.normal(0, 0.05, 2)))
        ref, ref_len, idx0, xy = _pack(rows)
        idx1, win = _run_fleet(solver, N, a, B, ref, ref_len, idx0, xy, limit=12)
        m = len(idx1)
        assert ((idx1 >= np.maximum(0, idx0[:m] - a)) & (idx1 < np.minimum(ref_len[:m], idx0[:m] + 5 * a))).all()
        short = ref_len[:m] < N
        assert short.any() and all(np.array_equal(win[i, -1], ref[i, ref_len[i] - 1]) for i in np.nonzero(short)[0])
    if B > 1:
        assert len(set(ref_len.tolist())) >= M - 8 and (idx1 != idx0).any()


@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("N,a", WINDOW_CASES)
def test_window_search_takes_the_first_of_two_equal_distances(N, a, B, solver20, solver40):
    """Exact ties.  (1) A straight dyadic reference and a state exactly midway between two neighbouring samples, offset in y:
    hypot(-1/8, dy) == hypot(1/8, dy) on either side.  The pair sits inside chunk 0, on lanes 63 | 64, inside the later chunks,
    and with its second sample as the last valid candidate (ub - 1, by the window's end and by the reference's end).  (2) A
    reference that goes out and comes back over the same samples: the nearest point is met twice, in different chunks.  The
    first candidate must win, like list.index(min(d))."""
    solver = solver20 if N == 20 else solver40
    lb, idx0, C = 3, a + 3, 6 * a
    rows, expect = [], []
    spots = sorted({j for j in (1, 62, 63, 64, 70, 126, 127, 128, 191, 192, 200, C - 2) if 0 <= j <= C - 2})
    for n, j in enumerate(spots):
        c = lb + j
        for clamp in (False, True):
            if clamp and c + 2 <= idx0:
                continue                                      # (the index must stay inside the reference)
            ref = _line(c + 2 if clamp else lb + C + 5)       # clamp: the later sample is the reference's last one
            rows.append((ref, idx0, (0.25 * c + 0.125, (0.375, 0.5, 1.0)[n % 3])))
            expect.append(c)
    pairs = [p for p in ((1, 3), (10, 64), (11, 65), (62, 64), (5, 75), (0, 118), (5, 201), (70, 130), (100, 230), (130, 200))
             if p[1] <= C - 1]
    for j1, j2 in pairs:
        T, n = lb + (j1 + j2) // 2, lb + C + 5
        k = np.arange(n)
        x = 0.25 * np.where(k <= T, k, 2 * T - k)             # out to sample T and back over the same points
        rows.append((np.stack([x, np.zeros(n), np.zeros(n)], axis=1), idx0, (0.25 * (lb + j1) + 0.0625, 0.375)))
        expect.append(lb + j1)
    ref, ref_len, idx, xy = _pack(rows)
    for i, r in enumerate(rows):                              # the cases are what they claim: two equal, smallest distances
        d = np.hypot(xy[i, 0] - r[0][lb:min(len(r[0]), lb + C), 0], xy[i, 1] - r[0][lb:min(len(r[0]), lb + C), 1])
        assert (d == d.min()).sum() == 2 and int(np.argmin(d)) == expect[i] - lb
    idx1, _ = _run_fleet(solver, N, a, B, ref, ref_len, idx, xy)
    assert np.array_equal(idx1, np.array(expect)[:len(idx1)])
    if a >= 11:
        assert any(e - lb >= 64 for e in expect) and any(e - lb == 63 for e in expect)


def test_tracker_view_with_action_steps_outside_1_to_N_is_refused_before_any_launch(solver20):
    for a in (0, 21):
        dev = DeviceTracker(make_cfg(20, action_steps=a), 2, solver=solver20)
        with pytest.raises(MpcGpuError):
            dev.local_refs()
        with pytest.raises(MpcGpuError):
            solver20.tracker_step(dev.view(), dev.refs, dev.out)


# ---- assembly: the comparisons on their thresholds ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 40])
def test_assembly_decides_like_the_host_on_the_thresholds(N, solver20, solver40):
    """goal = 0.  Robots 0..47: |x|, |y| in {0, 0.05, the double above 0.05} (<= 0.05 is near) and a last speed in {0.05, the double
    below it, -0.05, 0} (< 0.05 is slow): `active` must be what BatchedTracker.step's rule leaves.  Robots 48..63: on an axis
    at the distance d = base_speed * N * ts (evaluated in that order), its two neighbours and 0: the speed reference is the cap
    from d on (>=) and max(dist / N / ts, low_speed) below."""
    solver = solver20 if N == 20 else solver40
    cfg = make_cfg(N)
    B = 64
    host = BatchedTracker(cfg, B, solver=solver)
    dev = DeviceTracker(cfg, B, solver=solver)
    dev.view()
    rng = np.random.default_rng(N)
    up = np.nextafter(0.05, 1)
    xy = [(0.05, 0.0), (0.0, 0.05), (0.05, 0.05), (up, 0.0), (0.0, up), (up, up), (0.05, up), (up, 0.05), (-0.05, 0.05), (-up, 0.0),
          (0.0, -0.05), (-0.05, -up)]
    last = [0.05, np.nextafter(0.05, 0), -0.05, 0.0]
    for i in range(48):
        host.states[i, :2] = xy[i % 12]
        host.last_actions[i] = (last[i // 12], rng.normal())
    base = cfg.lin_vel_max * cfg.high_speed                   # work mode
    d = base * N * cfg.ts
    for i, dist in enumerate((d, np.nextafter(d, 0), np.nextafter(d, 2 * d), 0.0)):
        for j, axis in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
            host.states[48 + 4 * i + j, :2] = (axis[0] * dist, axis[1] * dist)
    host.last_actions[48:] = (0.3, 0.1)                       # moving: only the speed rule is at stake for these
    host.states[:, 2] = rng.uniform(-3, 3, B)
    refs_h = np.concatenate([rng.uniform(0, 10, (B, N, 2)), rng.uniform(-3, 3, (B, N, 1))], axis=2)
    refs_d = torch.from_numpy(refs_h).to(_dev())
    dev.states.copy_(torch.from_numpy(host.states)); dev.last_actions.copy_(torch.from_numpy(host.last_actions))
    P = host.assemble("work", refs_h)
    solver.debug_prep(P)
    want, rec = solver.debug_workspace(B)
    solver.debug_tracker_assemble(dev.view(), refs_d)
    got, _ = solver.debug_workspace(B)
    vref = slice(64, 64 + N)                                  # HDR doubles of header, then the speed references
    assert np.array_equal(np.delete(got[:, :rec], np.r_[vref], axis=1), np.delete(want[:, :rec], np.r_[vref], axis=1), equal_nan=True)
    assert np.allclose(got[:, vref], want[:, vref], rtol=4e-16, atol=0)
    capped = want[:, vref] == base
    assert np.array_equal(got[:, vref] == base, capped)
    # at d and above it the cap (>=); at 0 the floor; just below d the quotient (which may round to the cap: only the host decides)
    assert capped[48:52].all() and capped[56:60].all() and not capped[60:64].any()
    assert (got[60:64, vref] == cfg.low_speed).all() and (got[52:56, vref] > 0.999999 * base).all()
    # the termination test: the device's flags against what the host's step leaves (the rule of BatchedTracker.step itself)
    active_d = dev.active.cpu().numpy().astype(bool)
    host.step(refs=refs_h)
    assert np.array_equal(active_d, host.active)
    near = [i for i in range(48) if i % 12 in (0, 1, 2, 8, 10)]
    slow = [i for i in range(48) if i // 12 in (1, 3)]
    assert sorted(np.nonzero(~host.active)[0].tolist()) == sorted(set(near) & set(slow))


# ---- apply and rollout ----------------------------------------------------------------------------------------------------------
def _closed_loop(N, a, B, ticks, park):
    """DeviceTracker.step next to BatchedTracker.step on one handle.  The host's states are copied to the device after every tick
    (the rollouts differ by the last bits of sincos), so every tick compares like with like and the solves are bitwise equal."""
    cfg = make_cfg(N, action_steps=a, solver_max_inner_iterations=30, solver_max_outer_iterations=2)
    dev = DeviceTracker(cfg, B)
    host = BatchedTracker(cfg, B, solver=dev.solver)
    rng = np.random.default_rng(7 * N + a)
    for i in range(B):                                           # free corridor
        y = rng.uniform(3, 6)
        path = [(0.6, y), (14.0, y + rng.uniform(-1, 1))]
        start = np.array([0.6, y, rng.uniform(-0.2, 0.2)])
        for t in (host, dev):
            t.initialization(i, start, np.array([path[-1][0], path[-1][1], 0.0]), path)
    dev.view()
    worst_s = worst_p = 0.0
    parked = np.zeros(B, dtype=bool)
    sentinel = None
    for tick in range(ticks + 1):
        if tick == 1 and park:                                    # five robots exactly on their goals, standing still
            parked[[0, 5, 11, B - 2, B - 1]] = True
            host.states[parked, :2] = host.goals[parked, :2]
            host.last_actions[parked] = 0.0
            dev.states.copy_(torch.from_numpy(host.states)); dev.last_actions.copy_(torch.from_numpy(host.last_actions))
        if tick == ticks:                                         # one more step without the `actions` entry: actions_out is NULL
            sentinel = dev.out["actions"].fill_(NAN)              # the buffer the earlier ticks wrote: nobody may write it now
            dev.out = {k: v for k, v in dev.out.items() if k != "actions"}
        s0_h, s0_d = host.states.copy(), dev.states.cpu().numpy()
        p0_h, p0_d = host.pred_states.copy(), dev.pred_states.cpu().numpy()
        a_h, pred_h, cost_h = host.step()
        out = dev.step()
        torch.cuda.synchronize()
        u = out["u"].cpu().numpy()
        assert np.array_equal(u, host.last_result.solution), tick
        assert np.array_equal(out["status"].cpu().numpy(), host.last_result.status)
        assert np.array_equal(out["cost"].cpu().numpy(), cost_h)
        assert np.array_equal(dev.idx_ref.cpu().numpy(), host.idx_ref)
        act_d = dev.active.cpu().numpy().astype(bool)
        assert np.array_equal(act_d, host.active) and np.array_equal(~act_d, parked)
        u3 = u.reshape(B, N, 2)
        la_d, s_d, p_d = dev.last_actions.cpu().numpy(), dev.states.cpu().numpy(), dev.pred_states.cpu().numpy()
        assert np.array_equal(la_d, host.last_actions)
        assert np.array_equal(la_d[act_d], u3[act_d, a - 1]) and not la_d[~act_d].any()
        if "actions" in out:
            act = out["actions"].cpu().numpy()
            assert np.array_equal(act, a_h) and np.array_equal(act[act_d], u3[act_d, 0]) and not act[~act_d].any()
        else:
            assert np.isnan(sentinel.cpu().numpy()).all() and "actions" not in dev.out
        worst_s = max(worst_s, np.abs(s_d - host.states).max())
        worst_p = max(worst_p, np.abs(p_d - pred_h).max())
        assert np.abs(s_d - host.states).max() < 1e-12 and np.abs(p_d - pred_h).max() < 1e-11
        assert (np.abs(s_d - s0_d).max(axis=1)[act_d] > 0).all()      # whoever is active has moved
        # parked robots: state and prediction bitwise what they were, on both sides
        assert np.array_equal(s_d[~act_d], s0_d[~act_d]) and np.array_equal(host.states[~act_d], s0_h[~act_d])
        assert np.array_equal(p_d[~act_d], p0_d[~act_d]) and np.array_equal(host.pred_states[~act_d], p0_h[~act_d])
        dev.states.copy_(torch.from_numpy(host.states))
    print(f"\n[tracker limits] N = {N}, action_steps = {a}, {ticks + 1} ticks x {B} robots: bitwise equal solves; worst "
          f"|state_device - state_host| {worst_s:.2e} (bound 1e-12), worst |prediction_device - prediction_host| {worst_p:.2e} (bound 1e-11)")
    dev.solver.close()
    return parked


def test_apply_kernel_with_three_action_steps_and_parked_robots():
    parked = _closed_loop(20, 3, 37, 3, park=True)
    assert parked.sum() == 5


def test_apply_kernel_with_forty_action_steps():
    _closed_loop(40, 40, 3, 1, park=False)


# ---- proposal rollout -----------------------------------------------------------------------------------------------------------
_worst_rl = [0.0]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("ref_speed", [1.0, 0.0, -1.0])
@pytest.mark.parametrize("steps", [1, 20, 40])
@pytest.mark.parametrize("B", [1, 129])
def test_proposal_rollout_at_its_limits(B, steps, ref_speed, wide, solver20):
    """Every action; v and w start exactly on each limit, one accelerating step inside it and beyond it, so that both clamps act;
    ref_speed <= 0 takes SPEED_MAX; agent rows packed [B, 5] or the first five columns of the environment's 24-double state row.
    Tolerance 1e-12: the heading recursion has no transcendental and is identical on both sides; sincos differs by an ulp or two on
    values <= 1 that are scaled by ts * speed <= 0.3, over at most 40 steps of positions below 32 m."""
    ts = make_cfg(20).ts
    i = np.arange(B)
    dv, dw = ts * dqn.ACCELERATION_MAX, ts * dqn.ANGULAR_ACCELERATION_MAX
    v0 = np.array([dqn.SPEED_MAX, dqn.SPEED_MAX - dv, dqn.SPEED_MAX + 0.3, dqn.SPEED_MIN, dqn.SPEED_MIN + dv, dqn.SPEED_MIN - 0.3, 0.4])
    w0 = np.array([dqn.ANGULAR_VELOCITY_MAX, dqn.ANGULAR_VELOCITY_MAX - dw, dqn.ANGULAR_VELOCITY_MAX + 0.3, dqn.ANGULAR_VELOCITY_MIN,
                   dqn.ANGULAR_VELOCITY_MIN + dw, dqn.ANGULAR_VELOCITY_MIN - 0.3, 0.1])
    rng = np.random.default_rng(B + steps)
    action = i % 9 if B > 1 else np.array([0])                   # (B = 1: action 0 at both upper limits: both clamps act)
    agent = np.stack([rng.uniform(0, 16, B), rng.uniform(0, 16, B), rng.uniform(-3.2, 3.2, B), v0[i % 7], w0[(i // 2) % 7]], axis=1)
    # both clamps act on some rows (and leave others alone)
    v1 = agent[:, 3] + ts * np.where(action // 3 == 0, dqn.ACCELERATION_MAX, 0.0) + ts * np.where(action // 3 == 2, dqn.ACCELERATION_MIN, 0.0)
    w1 = agent[:, 4] + ts * np.where(action % 3 == 0, dqn.ANGULAR_ACCELERATION_MAX, 0.0) + ts * np.where(action % 3 == 2, dqn.ANGULAR_ACCELERATION_MIN, 0.0)
    assert (v1 > dqn.SPEED_MAX).any() and (w1 > dqn.ANGULAR_VELOCITY_MAX).any()
    if B > 1:
        assert (v1 < dqn.SPEED_MIN).any() and (w1 < dqn.ANGULAR_VELOCITY_MIN).any()
        assert (v1 == dqn.SPEED_MAX).any() and (v1 == dqn.SPEED_MIN).any() and ((v1 > dqn.SPEED_MIN) & (v1 < dqn.SPEED_MAX)).any()
        assert set(action.tolist()) == set(range(9))
    want, _ = dqn.rl_reference(agent, action, ts, steps=steps, ref_speed=ref_speed)
    if ref_speed <= 0.0 and steps > 1:
        other, _ = dqn.rl_reference(agent, action, ts, steps=steps, ref_speed=1.0)
        assert np.abs(other - want).max() > 0.01                 # the fallback speed is visible
    if wide:
        rows = torch.full((B + 1, 24), NAN, dtype=torch.float64, device=_dev())
        rows[:B, :5] = torch.from_numpy(agent).to(_dev())
        agent_d = rows[:B]
        assert agent_d.stride(0) == 24
    else:
        agent_d = torch.from_numpy(agent).to(_dev())
    out = torch.full((B + 1, steps, 2), NAN, dtype=torch.float64, device=_dev())
    solver20.rl_reference(agent_d, torch.from_numpy(action.astype(np.int64)).to(_dev()), ts, steps, ref_speed, LIMITS, out, stream=_stream())
    got = out.cpu().numpy()
    assert np.isnan(got[B]).all()                                # the sentinel row
    diff = np.abs(got[:B] - want).max()
    _worst_rl[0] = max(_worst_rl[0], diff)
    print(f"\n[tracker limits] proposal rollout B = {B}, steps = {steps}, ref_speed = {ref_speed}, wide = {wide}: max |device - host| "
          f"{diff:.2e}; worst so far {_worst_rl[0]:.2e} (bound 1e-12)")
    assert diff < 1e-12


def test_proposal_rollout_refuses_rows_narrower_than_five(solver20):
    agent = torch.zeros(4, 4, dtype=torch.float64, device=_dev())
    out = torch.full((4, 20, 2), NAN, dtype=torch.float64, device=_dev())
    with pytest.raises(MpcGpuError):
        solver20.rl_reference(agent, torch.zeros(4, dtype=torch.int64, device=_dev()), 0.2, 20, 1.0, LIMITS, out, stream=_stream())
    assert np.isnan(out.cpu().numpy()).all()


# ---- switcher kernel --------------------------------------------------------------------------------------------------------------
SWITCH = (10, 2, 1)         # switch below 10 m, count above 2 m, back after more than one counted tick


def switcher_ticks(B, N, S, O, with_live, ticks=15, V=8, seed=5):
    """Random geometry as in tests/test_gpu_device_tracker.py, `ticks` times: (polygons [B, O, V, 2], valid, positions [B, 3],
    original [B, N, 3], live or None).  With N > S a quarter of the fleet (another one every tick) has the first S rows of its
    reference far from every obstacle and the rows behind them inside obstacle 0, which is valid and near."""
    rng = np.random.default_rng(seed + 1000 * N + 10 * S + O)
    for tick in range(ticks):
        centres = rng.uniform(0, 12, (B, O, 1, 2))
        ang = np.sort(rng.uniform(0, 2 * np.pi, (B, O, V)), axis=2)
        rad = rng.uniform(0.3, 2.0, (B, O, V))
        poly = centres + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)
        poly[:, :, 6:] = poly[:, :, 5:6]                               # padded rings (repeated last vertex)
        valid = rng.random((B, O)) < 0.7
        pos = rng.uniform(0, 12, (B, 3))
        original = np.concatenate([rng.uniform(0, 12, (B, N, 2)), rng.uniform(-3, 3, (B, N, 1))], axis=2)
        if O:
            through = rng.random((B, 1, 1)) < 0.5
            original[:, :, :2] = np.where(through, centres[:, 0] + rng.normal(0, 0.2, (B, N, 2)), original[:, :, :2])
            if N > S:
                late = (np.arange(B) + tick) % 4 == 3
                original[late, :S, :2] = rng.uniform(40, 50, (int(late.sum()), S, 2))
                original[late, S:, :2] = centres[late, 0] + rng.normal(0, 0.05, (int(late.sum()), N - S, 2))
                valid[late, 0] = True
                pos[late, :2] = centres[late, 0, 0] + rng.uniform(-3, 3, (int(late.sum()), 2))
        live = rng.random(B) < 0.9 if with_live else None
        yield poly, valid, pos, original, live


@pytest.mark.parametrize("with_live", [True, False])
@pytest.mark.parametrize("O", [0, 6])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("N,S", [(40, 20), (20, 40), (20, 20)])
def test_switcher_kernel_with_proposals_of_another_length(N, S, B, O, with_live, solver20):
    """BatchSolver.hint_switch against BatchedHintSwitcher + tracked_reference, state carried over 15 ticks on both sides.  The
    proposal is the rollout kernel's own output (S rows), its host form dqn.rl_reference: proposal rows agree to 1e-12, every
    other row of `chosen` is bitwise the original reference.  Without obstacles (O = 0) nothing can change a switch: both sides
    start from the same random switch states and must keep them."""
    rng = np.random.default_rng(B + O)
    dev = _dev()
    ts = make_cfg(20).ts
    agent = np.stack([rng.uniform(0, 12, B), rng.uniform(0, 12, B), rng.uniform(-3, 3, B), rng.uniform(-0.5, 1.5, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    action = rng.integers(0, 9, B)
    want_rl, _ = dqn.rl_reference(agent, action, ts, steps=S, ref_speed=1.0)
    rl_ref = torch.empty(B, S, 2, dtype=torch.float64, device=dev)
    solver20.rl_reference(torch.from_numpy(agent).to(dev), torch.from_numpy(action).to(dev), ts, S, 1.0, LIMITS, rl_ref, stream=_stream())
    sw = hybrid.BatchedHintSwitcher(B, *SWITCH)
    if O == 0:
        sw.switch_on, sw.detach_cnt = rng.random(B) < 0.5, rng.integers(0, 5, B)
    first_on, first_cnt = sw.switch_on.copy(), sw.detach_cnt.copy()
    on_d = torch.from_numpy(sw.switch_on.astype(np.uint8)).to(dev)
    cnt_d = torch.from_numpy(sw.detach_cnt.astype(np.int32)).to(dev)
    chosen = torch.full((B + 1, N, 3), NAN, dtype=torch.float64, device=dev)
    seen_on = seen_off = late_robots = proposal_rows = 0
    common = min(N, S)
    for poly, valid, pos, original, live in switcher_ticks(B, N, S, O, with_live):
        prev = sw.switch_on.copy()
        on_h = sw.switch(pos[:, :2], original, poly, valid, live, proposal_rows=S)
        solver20.hint_switch(torch.from_numpy(poly).to(dev), torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(pos).to(dev),
                             torch.from_numpy(original).to(dev), rl_ref, None if live is None else torch.from_numpy(live.astype(np.uint8)).to(dev),
                             SWITCH, on_d, cnt_d, chosen, stream=_stream())
        got_on, got_c = on_d.cpu().numpy().astype(bool), chosen.cpu().numpy()
        assert np.array_equal(got_on, on_h)
        assert np.array_equal(cnt_d.cpu().numpy(), sw.detach_cnt)
        assert np.isnan(got_c[B]).all()                                  # the sentinel row
        use = on_h if live is None else on_h & live
        want_c = hybrid.tracked_reference(original, want_rl, use)
        prop = np.zeros((B, N), dtype=bool)
        prop[:, :common] = use[:, None]
        assert np.array_equal(got_c[:B][~prop], want_c[~prop]) and np.array_equal(got_c[:B][~prop], original[~prop])
        assert np.array_equal(got_c[:B, :, 2], original[:, :, 2])
        assert np.abs(got_c[:B] - want_c).max() < 1e-12
        proposal_rows += int(prop.sum())
        # robots whose reference enters an obstacle only on rows the proposal does not have: those rows switch nobody on
        inside = (hybrid.points_in_polygons(original[..., :2], poly) & valid[:, None, :]).any(axis=2)          # [B, N]
        late = ~inside[:, :common].any(axis=1) & inside[:, common:].any(axis=1) & (np.ones(B, bool) if live is None else live)
        late_robots += int(late.sum())
        assert not (late & ~prev & got_on).any() and not (late & ~prev & on_h).any()
        seen_on += int((on_h & ~prev).sum()); seen_off += int((~on_h & prev).sum())
    if O == 0:
        assert np.array_equal(sw.switch_on, first_on) and np.array_equal(sw.detach_cnt, first_cnt) and seen_on == seen_off == 0
    else:
        assert seen_on > 0 and seen_off > 0 and proposal_rows > 0      # both transitions, and rows of the proposal were tracked
        assert (late_robots > 0) == (N > S)


def test_switcher_kernel_thresholds_are_strict(solver20):
    """Distances that are exact in binary: the square's edge at x = 4, robots at x = 4 - 2 and a little to either side, switch and
    detach distance 2.  dist < switch_distance switches on, dist == switch_distance does not; dist > detach_distance counts,
    dist == detach_distance does not."""
    dev = _dev()
    B, N = 6, 20
    square = np.array([[4.0, 0.0], [6.0, 0.0], [6.0, 2.0], [4.0, 2.0]])
    poly = np.broadcast_to(square, (B, 1, 4, 2)).copy()
    valid = np.ones((B, 1), dtype=bool)
    x = np.array([2.0, 2.0 + 2.0 ** -40, 2.0 - 2.0 ** -40] * 2)
    pos = np.stack([x, np.ones(B), np.zeros(B)], axis=1)
    assert np.array_equal(hybrid.polygon_distances(pos[:, :2], poly)[:, 0] - 2.0 == 0, [True, False, False] * 2)
    original = np.zeros((B, N, 3))
    original[:3, :, :2] = (5.0, 1.0)                              # robots 0-2: the reference runs through the square, switch off
    original[3:, :, :2] = (9.0, 9.0)                              # robots 3-5: outside it, switch on
    start = np.array([False] * 3 + [True] * 3)
    sw = hybrid.BatchedHintSwitcher(B, 2.0, 2.0, 5)
    sw.switch_on = start.copy()
    on_h = sw.switch(pos[:, :2], original, poly, valid, None)
    on_d = torch.from_numpy(start.astype(np.uint8)).to(dev)
    cnt_d = torch.zeros(B, dtype=torch.int32, device=dev)
    rl_ref = torch.zeros(B, 20, 2, dtype=torch.float64, device=dev)
    chosen = torch.full((B + 1, N, 3), NAN, dtype=torch.float64, device=dev)
    solver20.hint_switch(torch.from_numpy(poly).to(dev), torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(pos).to(dev),
                         torch.from_numpy(original).to(dev), rl_ref, None, (2.0, 2.0, 5), on_d, cnt_d, chosen, stream=_stream())
    assert on_d.cpu().numpy().astype(bool).tolist() == on_h.tolist() == [False, True, False, True, True, True]
    assert cnt_d.cpu().numpy().tolist() == sw.detach_cnt.tolist() == [0, 0, 0, 0, 0, 1]
    assert np.isnan(chosen.cpu().numpy()[B]).all()


# ---- the whole tick at N_hor = 40 -----------------------------------------------------------------------------------------------
def test_device_tick_follows_the_host_tick_at_forty_steps():
    """DeviceHybrid next to BatchedHybrid with a 40-step horizon and the 20-step proposal: the rule of
    tests/test_gpu_hybrid.py::test_device_tick_follows_the_host_tick on the robots whose states still coincide."""
    dh = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.device_hybrid")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    loop = importlib.import_module("hybrid_loop")
    w = np.load(os.path.join(ROOT, "tests", "golden", "dqn_ray.npz"))
    q = dqn.QNetwork().load_arrays({k: w[k] for k in w.files if k.startswith("w")})
    cfg = make_cfg(40, solver_max_inner_iterations=30, solver_max_outer_iterations=2)
    rng = np.random.default_rng(3)
    B = 8
    scenes = [loop.scene(rng) for _ in range(B)]
    host = hybrid.BatchedHybrid(cfg, scenes, q, decision_mode=2)
    dev = dh.DeviceHybrid(cfg, scenes, q, decision_mode=2)
    together = np.ones(B, dtype=bool)
    n_compared = 0
    for tick in range(3):
        oh, od = host.tick(), dev.tick()
        gap = np.abs(oh["states"] - od["states"]).max(axis=1)
        together &= gap < 1e-6
        assert np.array_equal(oh["switch_on"][together], od["switch_on"][together]), tick
        assert np.array_equal(oh["done"][together], od["done"][together])
        n_compared += int(together.sum())
    assert dev._chosen.shape == (B, 40, 3) and dev._rl_ref.shape == (B, 20, 2)
    print(f"\n[tracker limits] device tick at N_hor = 40: robot-ticks compared on a common trajectory: {n_compared} of {3 * B}")
    assert n_compared > 0                                        # the two loops did run side by side
    host.tracker.solver.close(); dev.tracker.solver.close()
