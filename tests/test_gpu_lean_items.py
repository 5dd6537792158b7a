"""GPU (-m gpu): the lean item phase of the evaluation at N_hor = 20 (MPC_LEAN_ITEMS, csrc/mpc_kernels.hpp) against the former code,
which `make variants` keeps as libmpcgpu_items0.so.  The lean form takes the lane roles from 24-bit arithmetic, reads the cached
dynamic-row trips at compile-time distances from one lane base per table and the doubled weights of the gradient from LDS header
slots: no floating-point expression, order or contraction changes, so EVERY output bit must be the same --

  * the evaluation alone (mpcgpu_cost_grad_batch: psi, f, gradient, F1, F2; mpcgpu_psi_value_batch: the value-only form) on the
    reference vectors, the tie / kink vectors and random points over 0, 1, 3, 4, 7, 8, 9 and 10 dynamic rows (no trip, a partial
    trip, exactly the cached trips, the row loop beyond them), inside and outside hard and soft ellipses;
  * whole solves at the yaml's caps through the throughput kernel, and through the latency kernel by a forced tail promotion;
  * the kernels the knob does not reach (N_hor = 40, static slots of six edges): the same bits as well.
"""
import os

import numpy as np
import pytest

from conftest import load_golden, make_cfg
from support.edge_cases import KINDS, dyn_rows, table_kind
from test_gpu_value_only import _coverage
from trajtrack_mpcndqn_rlboost_amd import BatchSolver, scenes
from trajtrack_mpcndqn_rlboost_amd.solver import variant_path

pytestmark = pytest.mark.gpu

OLD = variant_path("items0")
FIELDS = ("solution", "cost", "status", "num_inner_iterations", "num_outer_iterations", "f2_norm")
SEEDS = {"benchmark": 17, "passing": 77, "avoidance": 27}
ROW_COUNTS = (0, 1, 3, 4, 7, 8, 9, 10)


def _need(lib):
    if not os.path.exists(lib):
        pytest.skip(f"{os.path.basename(lib)} not built (make variants)")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


# ---- the evaluation alone ---------------------------------------------------------------------------------------------------

def _assert_same_evaluation(cfg, u, p, c, y, what, **kw):
    """both hooks, the product build against libmpcgpu_items0.so; returns the shape the product build ran in"""
    _need(OLD)
    out = []
    for lib in (None, OLD):
        bs = BatchSolver(cfg, library=lib, **kw)
        r = bs.cost_grad(u, p, c, y)
        r["psi_value"] = bs.psi_value(u, p, c, y)
        out.append((r, bs.last_shape()))
        bs.close()
    (a, sa), (b, sb) = out
    for k in ("psi", "f", "grad", "F1", "F2", "psi_value"):
        bad = np.nonzero(_bits(a[k]) != _bits(b[k]))[0]
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {a[k].size} entries, first at {bad[0]}"
    assert np.isfinite(a["psi"]).all() and np.isfinite(a["grad"]).all(), what
    np.testing.assert_array_equal(_bits(a["psi"]), _bits(a["psi_value"]), err_msg=f"{what}: value-only psi")
    assert sa["lds_bytes"] == sb["lds_bytes"] and sa["waves_per_simd"] == sb["waves_per_simd"], (sa, sb)
    return sa


def test_evaluation_bitwise_on_the_reference_vectors():
    fx = load_golden("costgrad_N20.npz")
    cfg = make_cfg(20)
    _assert_same_evaluation(cfg, fx["u"], fx["p"], fx["c"], fx["y"], "costgrad_N20")
    _assert_same_evaluation(cfg, fx["u"], fx["p"], None, None, "costgrad_N20, c = 0")


def test_evaluation_bitwise_on_the_tie_and_kink_vectors_in_their_own_table_form():
    """the N_hor = 20 cases of costgrad_edges.npz, batched by table kind: the axis-aligned, rotated and general instantiations"""
    fx = load_golden("costgrad_edges.npz")
    cfg = make_cfg(20)
    n_p, n = cfg.num_params, 40
    rows = np.nonzero(fx["N"] == 20)[0]
    kind_of = np.array([table_kind(cfg, fx["p"][i, :n_p]) for i in rows])
    kinds = set()
    for kind in KINDS:
        sel = rows[kind_of == kind]
        if sel.size == 0:
            continue
        s = _assert_same_evaluation(cfg, fx["u"][sel, :n], fx["p"][sel, :n_p], fx["c"][sel], fx["y"][sel, :n], f"edges, {kind}")
        assert s["shape_const"] == (kind != "var") and s["axis_aligned"] == (kind == "axis"), (kind, s)
        kinds.add(kind)
    assert kinds == set(KINDS)


@pytest.mark.parametrize("family", ["benchmark", "avoidance"])
def test_evaluation_bitwise_on_random_points_over_the_dynamic_row_counts(family):
    """1024 seeded points: 128 per count of dynamic rows, rollouts of random inputs through the family's scenes"""
    N, per = 20, 128
    B = per * len(ROW_COUNTS)
    cfg = make_cfg(N)
    rng = np.random.default_rng(2000 + SEEDS[family])
    p = np.concatenate([scenes.make_family(cfg, per, family, n_dyn=kd, seed=SEEDS[family] + kd, n_other=2 * (kd % 2))["p"]
                        for kd in ROW_COUNTS])
    u = np.stack([rng.uniform(-0.5, 1.5, (B, N)), rng.uniform(-0.5, 0.5, (B, N))], axis=2).reshape(B, 2 * N)
    u[::16, 7] = rng.choice([-1.0, 1.0], B // 16) * rng.uniform(8.0, 12.0, B // 16)       # beyond the rollout's polynomial range
    c = 10.0 ** rng.integers(1, 7, B)
    y = rng.standard_normal((B, 2 * N)) * 10.0 ** rng.integers(-2, 3, (B, 1))
    kd = np.array([int(np.sum(np.any(dyn_rows(cfg, p[b]) != 0.0, axis=(1, 2)))) for b in range(B)])
    for want in ROW_COUNTS:
        assert np.sum(kd == want) == per, (want, np.bincount(kd))
    cov = _coverage(cfg, p, u)
    inside = cov["hard"] | cov["soft_only"]
    print(f"\n[{family}] inside a hard ellipse {int(cov['hard'].sum())}, a soft one only {int(cov['soft_only'].sum())}, outside every "
          f"ellipse with rows present {int(np.sum(~inside & (kd > 0)))}, polygon {int(cov['polygon'].sum())}, fleet disc {int(cov['fleet'].sum())}")
    for want in ROW_COUNTS[1:]:     # every row count has points inside a hard ellipse and points outside all of them
        assert (cov["hard"] & (kd == want)).any() and (~inside & (kd == want)).any(), want
    assert cov["soft_only"].any() and cov["polygon"].any() and cov["fleet"].any() and cov["plain_sincos"].any()
    s = _assert_same_evaluation(cfg, u, p, c, y, f"{family}, random points")
    assert s["max_dyn"] == max(ROW_COUNTS) and s["shape_const"] and s["axis_aligned"] and s["max_fleet"] == 2


# ---- whole solves -----------------------------------------------------------------------------------------------------------

def _solve(cfg, p, library=None, tail_promotion=0, **kw):
    bs = BatchSolver(cfg, latency_batch=0, order="as_given", tail_promotion=tail_promotion, library=library, **kw)
    r = bs.solve(p)
    ev = bs.last_eval_counts(p.shape[0])
    moved = bs.last_tail_promotion()[1]
    shape = bs.last_shape()
    bs.close()
    return r, ev, moved, shape


def _assert_same_solves(cfg, p, what, **kw):
    """the product build against libmpcgpu_items0.so: every output bit, both evaluation counters, the carve"""
    _need(OLD)
    a, ea, moved_a, sa = _solve(cfg, p, **kw)
    b, eb, moved_b, sb = _solve(cfg, p, library=OLD, **kw)
    print(f"\n[{what}] inner iterations median {np.median(a.num_inner_iterations):.0f} max {a.num_inner_iterations.max()}; promoted "
          f"{moved_a} / {moved_b}; LDS {sa['lds_bytes']} B, {sa['waves_per_simd']} wavefronts per SIMD")
    for f in FIELDS:
        np.testing.assert_array_equal(_bits(getattr(a, f)), _bits(getattr(b, f)), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(ea[0], eb[0], err_msg=f"{what}: psi evaluations")
    np.testing.assert_array_equal(ea[1], eb[1], err_msg=f"{what}: psi evaluations with gradient")
    assert sa["lds_bytes"] == sb["lds_bytes"] and sa["waves_per_simd"] == sb["waves_per_simd"], (sa, sb)
    return a, sa, moved_a


@pytest.mark.parametrize("stall", ["either", "both"])
@pytest.mark.parametrize("family", ["benchmark", "passing", "avoidance"])
def test_whole_solves_bitwise_against_the_former_item_phase(family, stall):
    cfg = make_cfg(20, solver_penalty_stall=stall)     # the yaml's own caps
    sc = scenes.make_family(cfg, 256, family, n_dyn=8, seed=SEEDS[family])
    _, s, _ = _assert_same_solves(cfg, sc["p"], f"{family}, {stall}")
    assert s["shape_const"] and s["axis_aligned"] and s["max_dyn"] == 8
    assert s["lds_bytes"] <= 10240 and s["waves_per_simd"] == 3     # a batch of 256 stays resident in the build without spills


def test_whole_solves_in_the_four_wavefront_build_bitwise_against_the_former_item_phase():
    """the benchmark's own instantiation (128 registers, four wavefronts per SIMD) is taken from 3073 problems on: 4096 short solves"""
    cfg = make_cfg(20, solver_max_inner_iterations=60, solver_max_outer_iterations=3)
    sc = scenes.make_family(cfg, 4096, "benchmark", n_dyn=8, seed=SEEDS["benchmark"])
    _, s, _ = _assert_same_solves(cfg, sc["p"], "benchmark, four wavefronts per SIMD")
    assert s["shape_const"] and s["axis_aligned"] and s["lds_bytes"] <= 10240 and s["waves_per_simd"] == 4


def test_solves_with_fleet_rows_bitwise_against_the_former_item_phase():
    cfg = make_cfg(20)
    sc = scenes.make_family(cfg, 256, "passing", n_dyn=8, seed=SEEDS["passing"], n_other=2)
    _, s, _ = _assert_same_solves(cfg, sc["p"], "2 fleet rows")
    assert s["max_fleet"] == 2


def _reshape_rows(cfg, p, general):
    """every dynamic row rotated (a constant angle per row: the shape-constant, non-axis-aligned instantiation); `general`: its
    semi-axes and angle also change with the step"""
    N = cfg.N_hor
    k = np.arange(N)
    for b in range(p.shape[0]):
        rows = dyn_rows(cfg, p[b])
        for i in np.nonzero(np.any(rows != 0.0, axis=(1, 2)))[0]:
            rows[i, :, 4] = 0.3 * (i + 1)
            if general:
                rows[i, :, 2] *= 1.0 + 0.01 * k
                rows[i, :, 3] *= 1.0 - 0.005 * k
                rows[i, :, 4] += 0.02 * k


@pytest.mark.parametrize("general", [False, True])
def test_solves_with_rotated_and_general_tables_bitwise_against_the_former_item_phase(general):
    cfg = make_cfg(20)
    sc = scenes.make_family(cfg, 256, "benchmark", n_dyn=8, seed=31)
    _reshape_rows(cfg, sc["p"], general)
    _, s, _ = _assert_same_solves(cfg, sc["p"], "general tables" if general else "rotated ellipses")
    assert s["shape_const"] == (not general) and not s["axis_aligned"]


def test_promoted_solves_bitwise_against_the_former_item_phase():
    """every problem of a small batch is promoted once the first has finished: they finish in the latency kernel, which shares the
    evaluation's source; promotion on against off, exact as well"""
    B = 64
    cfg = make_cfg(20)
    sc = scenes.make_family(cfg, B, "passing", n_dyn=8, seed=SEEDS["passing"])
    a, _, moved = _assert_same_solves(cfg, sc["p"], "tail promotion", tail_promotion=B)
    assert moved > 0
    off, _, _, _ = _solve(cfg, sc["p"])
    for f in FIELDS:
        np.testing.assert_array_equal(_bits(getattr(a, f)), _bits(getattr(off, f)), err_msg=f"promotion on / off: {f}")


# ---- the kernels the knob does not reach --------------------------------------------------------------------------------------

def test_long_horizon_solves_keep_their_bits():
    cfg = make_cfg(40, solver_max_inner_iterations=30, solver_max_outer_iterations=2)
    sc = scenes.make_batch(cfg, 64, n_dyn=8, seed=78)
    _assert_same_solves(cfg, sc["p"], "N_hor = 40")


def test_solves_with_six_edge_static_slots_keep_their_bits():
    """nstcobs = 18: the generic-horizon kernels (static slots wider than the compiled four edges)"""
    cfg = make_cfg(20, nstcobs=18, solver_max_inner_iterations=60, solver_max_outer_iterations=3)
    sc = scenes.make_family(cfg, 64, "passing", n_dyn=3, seed=420)
    _assert_same_solves(cfg, sc["p"], "nstcobs = 18")
