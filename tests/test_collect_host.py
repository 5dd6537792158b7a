"""Collection inside one launch without a GPU: the binding table of ``collect`` and its header, every refusal
of the two entries from a process that never touches a device, the numpy twin of the action rule
(tests/support/collect_numpy.py) against integer and rational arithmetic, its greedy actions against the float64 Q-network,
and the refusals of ``DqnLearner(collect_in_kernel=True)`` and the training tool."""
import ctypes as C
import importlib
import os
import re
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from support import collect_numpy as cn, dqn_cases, dqn_numpy as tw
from trajtrack_mpcndqn_rlboost_amd import collect, dqn, dqn_fused, dqn_train, rl_env

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mpcgpu_[a-z_0-9]+)\s*\(", text))


# ---- binding ---------------------------------------------------------------------------------------------------------------
def test_the_built_library_and_the_header_have_exactly_these_exports():
    path = solver_mod.library_path()
    assert os.path.exists(path), f"{path} missing -- run __graft_entry__.build()"
    lib = C.CDLL(path)
    for sym in collect.COLLECT_EXPORTS:
        assert hasattr(lib, sym), sym
    lib.mpcgpu_abi_version.restype = C.c_int32
    assert lib.mpcgpu_abi_version() == 8
    assert declared("mpcgpu_collect.h") == set(collect.COLLECT_EXPORTS)
    for header in ("mpcgpu_env.h", "mpcgpu_dqn.h", "mpcgpu_dqn_per.h", "mpcgpu_map.h"):
        assert not declared(header) & set(collect.COLLECT_EXPORTS), header
    text = open(os.path.join(ROOT, "include", "mpcgpu_collect.h")).read()
    assert int(re.search(r"#define MPCGPU_COLLECT_MAX_STEPS (\d+)", text).group(1)) == collect.MAX_STEPS == 64
    assert C.sizeof(collect._CCollectParams) == 8 * 64 + 8 * 4 + 4 * 2


# ---- refusals of the entries: no device is touched ---------------------------------------------------------------------------
def env_params(**kw):
    base = dict(n_path_max=4, n_obst_max=2, n_kf_max=2, n_edge_max=16, num_segments=8, corner_samples=3, time_step=0.2,
                sample_offset=0.0, collision_factor=4.0, reach_goal_factor=3.0, cross_track_factor=0.05,
                excessive_speed_factor=4.0, reference_speed=1.2, path_progress_factor=2.0, **rl_env.ROBOT)
    base.update(kw)
    return rl_env._CParams(**base)


def collect_params(T=4, capacity=64, pos0=0, eps=None):
    p = collect._CCollectParams(seed=1, serial0=0, capacity=capacity, pos0=pos0, T=T)
    for t, e in enumerate([0.5] * 64 if eps is None else eps):
        p.eps[t] = e
    return p


def test_refusals_of_the_entries_need_no_device():
    """Every refusal comes before the device is touched (this process has none), with this module's own error text."""
    lib = collect._bind(solver_mod.load_library())
    p = 4096                                                       # any non-null address: a refused call reads none of them
    env_ptrs = ["records", "state", "obs_internal", "obs_external", "reward", "terminated", "truncated", "term_internal", "term_external"]
    ring_ptrs = ["theta", "buf_obs", "buf_next_obs", "buf_actions", "buf_rewards", "buf_dones", "ep_return"]

    def rays(params=None, B=8, max_steps=3, cp=None, **null):
        a = {k: (None if k in null else p) for k in env_ptrs + ring_ptrs}
        params = env_params() if params is None else params
        cp = collect_params() if cp is None else cp
        return lib.mpcgpu_collect_rays_dev(
            0, C.byref(params) if params != "null" else None, B, *(a[k] for k in env_ptrs), max_steps, a["theta"],
            C.byref(cp) if cp != "null" else None, *(a[k] for k in ring_ptrs[1:]), None, None, None, None, None)
    nan = float("nan")
    cases = [(dict(**{k: True}), "null pointer") for k in env_ptrs + ring_ptrs]
    cases += [(dict(cp="null"), "null pointer"), (dict(params="null"), "invalid mpcgpu_env_params"),
              (dict(cp=collect_params(T=0)), "1 <= T <= 64"), (dict(cp=collect_params(T=65, capacity=10 ** 6)), "1 <= T <= 64"),
              (dict(cp=collect_params(T=-1)), "1 <= T <= 64"),
              (dict(cp=collect_params(T=4, capacity=31)), "T * B must not exceed capacity"),
              (dict(cp=collect_params(T=64, capacity=511)), "T * B must not exceed capacity"),
              (dict(cp=collect_params(capacity=0)), "0 <= pos0 < capacity"), (dict(cp=collect_params(pos0=64)), "0 <= pos0 < capacity"),
              (dict(cp=collect_params(pos0=-1)), "0 <= pos0 < capacity"),
              (dict(max_steps=0), "max_episode_steps must be positive"), (dict(max_steps=-5), "max_episode_steps must be positive"),
              (dict(cp=collect_params(eps=[0.5, 0.5, 0.5, 1.0 + 2.0 ** -52])), "must lie in [0, 1]"),
              (dict(cp=collect_params(eps=[0.5, -1e-300, 0.5, 0.5])), "must lie in [0, 1]"),
              (dict(cp=collect_params(eps=[nan, 0.5, 0.5, 0.5])), "must lie in [0, 1]"),
              (dict(cp=collect_params(eps=[0.5, 0.5, 0.5, float("inf")])), "must lie in [0, 1]"),
              (dict(B=-1), "negative batch"),
              (dict(params=env_params(n_path_max=65)), "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
              (dict(params=env_params(n_obst_max=32)), "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
              (dict(params=env_params(n_edge_max=0)), "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)"),
              (dict(params=env_params(num_segments=16)), "only num_segments = 8 and corner_samples = 3 are built"),
              (dict(params=env_params(corner_samples=2)), "only num_segments = 8 and corner_samples = 3 are built")]
    for kw, text in cases:
        assert rays(**kw) < 0 and text in lib.mpcgpu_collect_last_error().decode(), (kw, lib.mpcgpu_collect_last_error())
    # an eps beyond T is not read; an empty batch is nothing to do
    assert rays(B=0, cp=collect_params(T=2, eps=[0.0, 1.0, nan, 7.0])) == 0
    # the words of the environment's own entry for the same params
    env_lib = rl_env._bind(lib)
    bad = env_params(num_segments=16)
    assert env_lib.mpcgpu_env_step_autoreset_dev(0, C.byref(bad), 8, p, p, p, p, p, p, p, p, p, p, 3, None) < 0
    assert rays(params=bad) < 0 and lib.mpcgpu_collect_last_error() == env_lib.mpcgpu_env_last_error()

    def act(theta=p, ext=p, inte=p, B=8, eps=0.5, actions=p):
        return lib.mpcgpu_collect_act_dev(0, theta, ext, inte, B, eps, 1, 0, actions, None, None)
    for kw, text in ((dict(theta=None), "null pointer"), (dict(ext=None), "null pointer"), (dict(inte=None), "null pointer"),
                     (dict(actions=None), "null pointer"), (dict(B=-1), "negative batch"), (dict(eps=nan), "eps must lie in [0, 1]"),
                     (dict(eps=-0.1), "eps must lie in [0, 1]"), (dict(eps=1.5), "eps must lie in [0, 1]")):
        assert act(**kw) < 0 and text in lib.mpcgpu_collect_last_error().decode(), kw
    assert act(B=0) == 0


def _stub_env(**kw):
    return types.SimpleNamespace(B=4, device=torch.device("cpu"), is_image_env=False, image_shape=(3, 54, 54), **kw)


def test_python_refuses_the_image_and_the_fresh_map_environment():
    with pytest.raises(ValueError, match="ray environment only"):
        collect.check_env(types.SimpleNamespace(is_image_env=True))
    with pytest.raises(ValueError, match="enable_spares"):
        collect.check_env(types.SimpleNamespace(is_image_env=False, records2=torch.zeros(2, 1, 4)))
    collect.check_env(types.SimpleNamespace(is_image_env=False, records2=None))
    with pytest.raises(ValueError, match="ray environment only"):
        dqn_train.DqnLearner(types.SimpleNamespace(B=4, device=torch.device("cpu"), is_image_env=True, image_shape=(3, 54, 54)),
                             buffer_size=8, collect_in_kernel=True)
    with pytest.raises(ValueError, match="enable_spares"):
        dqn_train.DqnLearner(_stub_env(records2=torch.zeros(2, 4, 4)), buffer_size=8, collect_in_kernel=True)
    with pytest.raises(ValueError, match="collect_launch_steps"):
        dqn_train.DqnLearner(_stub_env(), buffer_size=8, collect_in_kernel=True, collect_launch_steps=0)


def test_collect_in_kernel_is_off_by_default_and_keeps_the_checkpoint_keys():
    off = dqn_train.DqnLearner(_stub_env(), buffer_size=8, seed=3)
    assert off.collect_in_kernel is False
    assert not {"collect_seed", "collect_serial"} & set(off.state_dict())
    on = dqn_train.DqnLearner(_stub_env(), buffer_size=8, seed=3, collect_in_kernel=True, train_freq=100)
    d = on.state_dict()
    assert set(d) - set(off.state_dict()) == {"collect_seed", "collect_serial"}
    assert d["collect_serial"] == 0 and d["collect_seed"] != 3 and 0 <= d["collect_seed"] < 2 ** 64
    assert on.collect_launch_steps == 64                  # a round of 100 steps is split, not refused
    assert dqn_train.DqnLearner(_stub_env(), buffer_size=8, collect_in_kernel=True, collect_launch_steps=5).collect_launch_steps == 5
    on.collect_serial = 17
    other = dqn_train.DqnLearner(_stub_env(), buffer_size=8, seed=9, collect_in_kernel=True)
    other.load_state_dict(on.state_dict())
    assert (other.collect_seed, other.collect_serial) == (on.collect_seed, 17)
    for seed in range(50):                                # exploration never shares the stream of the minibatch rows (seed + rank)
        assert dqn_train.DqnLearner(_stub_env(), buffer_size=8, seed=seed, collect_in_kernel=True).collect_seed != seed


def test_training_tool_takes_collect_in_kernel():
    sys.path.insert(0, ROOT)
    train_dqn = importlib.import_module("tools.train_dqn")
    assert train_dqn.parse_args(["--collect-in-kernel", "--fused"]).collect_in_kernel
    assert not train_dqn.parse_args([]).collect_in_kernel
    for argv in (["--collect-in-kernel", "--images"], ["--collect-in-kernel", "--fresh-maps"]):
        with pytest.raises(SystemExit) as err:
            train_dqn.parse_args(argv)
        assert err.value.code == 2


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def test_draws_are_exact_integer_arithmetic():
    rng = np.random.default_rng(5)
    pairs = [(0, 0), (2 ** 40, 0), (2 ** 64 - 1, 2 ** 31 - 1)] + [(int(s), int(b)) for s, b in
                                                               zip(rng.integers(0, 2 ** 62, 10 ** 4), rng.integers(0, 2 ** 20, 10 ** 4))]
    seed = 0x1234_5678_9ABC_DEF0
    seen = set()
    for serial, b in pairs:
        bits_e, bits_a = cn.draw_bits(seed, serial, b)
        u, r = cn.uniform_of(bits_e), cn.random_of(bits_a)
        assert Fraction(u) == Fraction(bits_e >> 11, 2 ** 53) and 0.0 <= u < 1.0
        assert r == bits_a * 9 // 2 ** 64 and 0 <= r <= 8
        assert not (u < 0.0) and u < 1.0                                   # eps = 0 never explores, eps = 1 always does
        assert bits_e != bits_a
        seen.add(r)
    assert seen == set(range(9))
    assert cn.uniform_of(2 ** 64 - 1) == 1.0 - 2.0 ** -53 and cn.uniform_of(2 ** 11 - 1) == 0.0
    assert cn.random_of(2 ** 64 - 1) == 8 and cn.random_of(0) == 0
    # the stream of the fused trainer's minibatch rows with the same (seed, serial) uses the multipliers i + 1 = 1 .. n: the
    # draws of row b are its entries 2 b and 2 b + 1, which is why the learner gives collection a seed of its own
    for serial in (0, 7, 2 ** 40):
        key = tw.mix64((seed + tw._G * serial) & tw._MASK)
        for b in (0, 1, 300):
            e, a = cn.draw_bits(seed, serial, b)
            assert e == tw.mix64((key + tw._G * (2 * b + 1)) & tw._MASK) and a == tw.mix64((key + tw._G * (2 * b + 2)) & tw._MASK)
        rows = tw.sample_rows(seed ^ 0x436F6C6C65637421, serial, 64, 2 ** 31 - 1).tolist()
        mine = [(x * (2 ** 31 - 1)) >> 64 for b in range(32) for x in cn.draw_bits(seed, serial, b)]
        assert not set(rows) & set(mine)


def test_epsilon_ends_and_tie_rule_of_the_twin():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (300, 46)).astype(F)
    theta = dqn_cases.random_theta(rng)
    a0, q, e0, u = cn.act(theta, x, 0.0, 11, 5)
    a1, _, e1, _ = cn.act(theta, x, 1.0, 11, 5)
    assert not e0.any() and e1.all() and u.max() < 1.0
    assert np.array_equal(a0, cn.greedy(q)) and len(set(a0.tolist())) > 1
    assert np.array_equal(a1, [cn.random_of(cn.draw_bits(11, 5, b)[1]) for b in range(300)]) and set(a1.tolist()) == set(range(9))
    mid, _, em, _ = cn.act(theta, x, 0.3, 11, 5)
    assert 0 < em.sum() < 300 and np.array_equal(em, u < 0.3) and np.array_equal(mid, np.where(em, a1, a0))
    # all-zero theta: nine equal values, the scan keeps index 0
    az, qz, _, _ = cn.act(np.zeros(tw.NP, F), x, 0.0, 11, 5)
    assert not qz.any() and not az.any()
    # output rows 3 and 7 are copies and carry the largest bias: q[3] == q[7] is the maximum in every row, the scan keeps 3
    tied = dqn_cases.random_theta(rng)
    W2, b2 = tw.split(tied)[4:]
    W2[7] = W2[3]
    b2[:] = 0.0
    b2[[3, 7]] = 50.0
    at, qt, _, _ = cn.act(tied, x, 0.0, 11, 5)
    assert np.array_equal(qt[:, 3], qt[:, 7]) and (qt.max(axis=1) == qt[:, 3]).all() and (at == 3).all()


def test_greedy_actions_of_the_twin_against_the_float64_network():
    """Two float32 evaluations (the twin's sequential sums, torch's own) each deviate from float64 by some largest amount; on every
    row whose float64 margin between best and second exceeds the sum of the two, all three pick the same action."""
    rng = np.random.default_rng(2024)
    theta = dqn_cases.random_theta(rng)
    x = rng.uniform(-1, 1, (1000, 46)).astype(F)
    net64, net32 = dqn.QNetwork().double(), dqn.QNetwork()
    for net, dtype in ((net64, torch.float64), (net32, torch.float32)):
        off = 0
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(torch.from_numpy(theta[off:off + p.numel()].astype(np.float64)).reshape(p.shape).to(dtype))
                off += p.numel()
    with torch.no_grad():
        q64 = net64(torch.from_numpy(x).double()).numpy()
        q32 = net32(torch.from_numpy(x)).numpy()
    want = net64.greedy_actions(torch.from_numpy(x).double()).numpy()
    mine, q, _, _ = cn.act(theta, x, 0.0, 1, 0)
    dev_twin, dev_torch = np.abs(q.astype(np.float64) - q64).max(), np.abs(q32.astype(np.float64) - q64).max()
    assert 0.0 < dev_twin < 1e-5 and 0.0 < dev_torch < 1e-5
    top = np.sort(q64, axis=1)
    clear = (top[:, -1] - top[:, -2]) > dev_twin + dev_torch
    print(f"deviation from float64: twin {dev_twin:.3e}, torch float32 {dev_torch:.3e}; {int(clear.sum())} of 1000 rows are clear")
    assert clear.sum() >= 950
    assert np.array_equal(mine[clear], want[clear])
    assert np.array_equal(net32.greedy_actions(torch.from_numpy(x)).numpy()[clear], want[clear])
