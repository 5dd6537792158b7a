"""GPU (-m gpu): the value-only form of the evaluation (eval_point's template parameter VO, MPC_VALUE_ONLY in
csrc/mpc_kernels.hpp), which the Lipschitz test of the throughput kernel's step loop runs, against the general form with
want_grad = false -- the build `make variants` keeps as libmpcgpu_vo0.so.  The value-only form leaves out every gradient partial
and keeps every expression psi is made of, so

  * psi of the value-only hook (mpcgpu_psi_value_batch) equals psi of the cost/gradient hook BIT FOR BIT -- on the reference
    vectors (ties and kinks included) and on seeded random points around the families' cold-start iterates whose coverage of the
    evaluation's branches (hard / soft ellipse, polygon, fleet disc, plain sincos path) is asserted;
  * whole solves give every output bit and both evaluation counters of libmpcgpu_vo0.so, with the same LDS carve and residency.

The Lipschitz psi only feeds a comparison: a last-place error there can leave whole solves unchanged, hence the direct check.
The hook is a kernel of its own: it always instantiates the value-only form as eval_point<..., MINW = 3, VO = true>, while the
benchmark's solve kernel inlines a four-wavefront copy at its Lipschitz site.  The direct check therefore pins the value-only
SOURCE, not that inlined copy; that the two instantiations give the same bits rests on -ffp-contract=on (an expression is fused as
written, whatever it is inlined into) together with the whole-solve tests below, which run the inlined copies themselves.
"""
import os

import numpy as np
import pytest

from conftest import load_golden, make_cfg
from support.edge_cases import KINDS, dyn_rows, table_kind
from trajtrack_mpcndqn_rlboost_amd import BatchSolver, scenes
from trajtrack_mpcndqn_rlboost_amd.solver import variant_path

pytestmark = pytest.mark.gpu

OLD = variant_path("vo0")
FIELDS = ("solution", "cost", "status", "num_inner_iterations", "num_outer_iterations", "f2_norm", "last_problem_norm_fpr",
          "lagrange_multipliers")
SEEDS = {"benchmark": 17, "passing": 77, "avoidance": 27}
K_SMALL = 0.78          # |half-step heading increment| up to which the rollout uses its polynomials (KTAB[15])


def _need(lib):
    if not os.path.exists(lib):
        pytest.skip(f"{os.path.basename(lib)} not built (make variants)")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


# ---- psi alone --------------------------------------------------------------------------------------------------------------

def _assert_psi_bits(bs, u, p, c, y, what):
    full = bs.cost_grad(u, p, c, y)["psi"]
    vo = bs.psi_value(u, p, c, y)
    bad = np.nonzero(_bits(full) != _bits(vo))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(full)} differ, first {bad[0]}: {full[bad[0]]!r} vs {vo[bad[0]]!r}"
    assert np.isfinite(full).all(), what
    return full


@pytest.mark.parametrize("N", [20, 40])
def test_psi_bitwise_on_the_reference_vectors(N):
    fx = load_golden(f"costgrad_N{N}.npz")
    for pairing in ((None, 2) if N == 20 else (None,)):
        bs = BatchSolver(make_cfg(N), pairing=pairing)
        _assert_psi_bits(bs, fx["u"], fx["p"], fx["c"], fx["y"], f"costgrad_N{N} pairing={pairing}")
        _assert_psi_bits(bs, fx["u"], fx["p"], None, None, f"costgrad_N{N} pairing={pairing}, c = 0")
        assert bs.last_shape()["problems_per_wavefront"] == (pairing or 1)
        bs.close()


def test_psi_bitwise_on_the_edge_vectors_in_their_own_table_form():
    """Every case of costgrad_edges.npz (exact ties of the path minimum, kinks, horizons 2-64), batched by horizon and table kind
    so that the axis-aligned, rotated and general forms of the evaluation all run; N_hor = 20 also two problems per wavefront."""
    fx = load_golden("costgrad_edges.npz")
    seen, kinds = 0, set()
    for N in sorted({int(n) for n in fx["N"]}):
        cfg = make_cfg(N)
        n_p, n = cfg.num_params, 2 * N
        rows = np.nonzero(fx["N"] == N)[0]
        kind_of = np.array([table_kind(cfg, fx["p"][i, :n_p]) for i in rows])
        for pairing in ((None, 2) if N == 20 else (None,)):
            bs = BatchSolver(cfg, pairing=pairing)
            for kind in KINDS:
                sel = rows[kind_of == kind]
                if sel.size == 0:
                    continue
                _assert_psi_bits(bs, fx["u"][sel, :n], fx["p"][sel, :n_p], fx["c"][sel], fx["y"][sel, :n],
                                 f"edges N={N} {kind} pairing={pairing}")
                s = bs.last_shape()
                assert s["shape_const"] == (kind != "var") and s["axis_aligned"] == (kind == "axis"), (kind, s)
                kinds.add(kind)
                seen += sel.size if pairing is None else 0
            bs.close()
    assert seen == len(fx["N"]) and kinds == set(KINDS)


def _coverage(cfg, p, u):
    """Which branches of the evaluation the points (p, u) take -- a plain numpy rollout (Simpson rule of the position integral,
    as the kernel's) and the indicator functions of mpc_generator.py; margins of 1e-9 keep rounding out of the classification."""
    N, ts, off = cfg.N_hor, cfg.ts, cfg.offsets()
    B = p.shape[0]
    v, w = u[:, 0::2], u[:, 1::2]
    th1 = p[:, 2:3] + np.cumsum(ts * w, axis=1)
    th0 = th1 - ts * w
    thm = th0 + 0.5 * ts * w
    X = p[:, 0:1] + np.cumsum(ts * v * (np.cos(th0) + 4.0 * np.cos(thm) + np.cos(th1)) / 6.0, axis=1)
    Y = p[:, 1:2] + np.cumsum(ts * v * (np.sin(th0) + 4.0 * np.sin(thm) + np.sin(th1)) / 6.0, axis=1)
    eps = 1e-9
    dyn = p[:, off["od"]:off["od"] + cfg.Ndynobs * 6 * N].reshape(B, cfg.Ndynobs, N, 6)
    act = np.any(dyn != 0.0, axis=(2, 3))[:, :, None]
    ex, ey = X[:, None, :] - dyn[..., 0], Y[:, None, :] - dyn[..., 1]
    ca, sa = np.cos(dyn[..., 4]), np.sin(dyn[..., 4])
    a2, b2 = (ex * ca + ey * sa) ** 2, (ex * sa - ey * ca) ** 2
    hard = 1.0 - a2 / (dyn[..., 2] + 1e-6) ** 2 - b2 / (dyn[..., 3] + 1e-6) ** 2
    soft = 1.0 - a2 / (dyn[..., 2] + cfg.social_margin + 1e-6) ** 2 - b2 / (dyn[..., 3] + cfg.social_margin + 1e-6) ** 2
    in_hard = np.any(act & (hard > eps), axis=(1, 2))
    in_soft = np.any(act & (soft > eps) & (dyn[..., 5] * p[:, None, off["qdyn"]:off["qdyn"] + N] > 0.0), axis=(1, 2))
    soft_only = in_soft & ~np.any(act & (hard > -eps), axis=(1, 2))
    stc = p[:, off["os"]:off["os"] + cfg.Nstcobs * 12].reshape(B, cfg.Nstcobs, 12)
    h = stc[:, :, None, 0:4] - stc[:, :, None, 4:8] * X[:, None, :, None] - stc[:, :, None, 8:12] * Y[:, None, :, None]
    in_poly = np.any(np.any(stc != 0.0, axis=2)[:, :, None] & (h.min(axis=3) > eps), axis=(1, 2))
    flt = p[:, off["c"]:off["c"] + cfg.Nother * 3 * N].reshape(B, cfg.Nother, N, 3)
    fact = np.any(flt != 0.0, axis=(2, 3))[:, :, None]
    d2 = (X[:, None, :] - flt[..., 0]) ** 2 + (Y[:, None, :] - flt[..., 1]) ** 2
    in_fleet = np.any(fact & (cfg.vehicle_width ** 2 - d2 > eps), axis=(1, 2))
    plain = np.any(0.5 * ts * np.abs(w) > K_SMALL * (1.0 + 1e-9), axis=1)
    return dict(hard=in_hard, soft_only=soft_only, polygon=in_poly, fleet=in_fleet, plain_sincos=plain,
                fleet_rows=bool(fact.any()))


@pytest.mark.parametrize("family,n_other", [("benchmark", 0), ("benchmark", 2), ("passing", 2), ("avoidance", 2)])
def test_psi_bitwise_on_random_points_around_the_cold_start_iterates(family, n_other):
    """4096 seeded points per family (N_hor = 20, 8 dynamic rows, 5 static): the iterate of a cold-started solve after 0-12 PANOC
    steps of its first inner problem plus noise of 1e-3 .. 1 (log-uniform per point); one point in eight carries angular speeds
    beyond the polynomial range of the rollout (0.5 ts |w| > 0.78).  Penalties 10 .. 1e6 and random multipliers."""
    B, N = 4096, 20
    rng = np.random.default_rng(1000 + SEEDS[family] + n_other)
    sc = scenes.make_family(make_cfg(N), B, family, n_dyn=8, seed=SEEDS[family], n_other=n_other)
    u = np.zeros((B, 2 * N))
    for j, steps in enumerate((4, 12)):          # a third of the points stays at the cold start u = 0 itself
        cfg = make_cfg(N, solver_max_inner_iterations=steps, solver_max_outer_iterations=1)
        bs = BatchSolver(cfg, latency_batch=0, tail_promotion=0)
        sel = np.arange(B) % 3 == j + 1
        u[sel] = bs.solve(sc["p"][sel]).solution
        bs.close()
    u += np.exp(rng.uniform(np.log(1e-3), np.log(1.0), (B, 1))) * rng.standard_normal((B, 2 * N))
    wide = np.arange(B) % 8 == 5
    big = rng.random((B, N)) < 0.15
    big[:, 3] = True
    u[:, 1::2] = np.where(wide[:, None] & big, rng.choice([-1.0, 1.0], (B, N)) * rng.uniform(8.0, 12.0, (B, N)), u[:, 1::2])
    c = 10.0 ** rng.integers(1, 7, B)
    y = rng.standard_normal((B, 2 * N)) * 10.0 ** rng.integers(-2, 3, (B, 1))
    cfg = make_cfg(N)
    cov = _coverage(cfg, sc["p"], u)
    print(f"\n[{family}, {n_other} fleet rows] " + ", ".join(f"{k} {int(np.sum(v))}" for k, v in cov.items() if k != "fleet_rows"))
    assert cov["hard"].any() and cov["soft_only"].any() and cov["polygon"].any() and cov["plain_sincos"].any()
    assert cov["fleet_rows"] == (n_other > 0) and (cov["fleet"].any() or not cov["fleet_rows"])
    bs = BatchSolver(cfg)
    _assert_psi_bits(bs, u, sc["p"], c, y, f"{family} random points")
    s = bs.last_shape()
    assert s["max_dyn"] == 8 and s["max_static"] == 5 and s["max_fleet"] == n_other
    bs.close()


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
    """the product build against libmpcgpu_vo0.so: every output bit, both counters, the carve; every problem ran Lipschitz tests"""
    _need(OLD)
    a, ea, moved_a, sa = _solve(cfg, p, **kw)
    b, eb, moved_b, sb = _solve(cfg, p, library=OLD, **kw)
    print(f"\n[{what}] inner iterations median {np.median(a.num_inner_iterations):.0f} max {a.num_inner_iterations.max()}; "
          f"gradient-free evaluations per problem min {int((ea[0] - ea[1]).min())}; promoted {moved_a} / {moved_b}; "
          f"LDS {sa['lds_bytes']} B, {sa['waves_per_simd']} wavefronts per SIMD")
    for f in FIELDS:
        np.testing.assert_array_equal(_bits(getattr(a, f)), _bits(getattr(b, f)), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(ea[0], eb[0], err_msg=f"{what}: psi evaluations")
    np.testing.assert_array_equal(ea[1], eb[1], err_msg=f"{what}: psi evaluations with gradient")
    assert ((ea[0] - ea[1]) > 0).all(), what
    assert sa["lds_bytes"] == sb["lds_bytes"] and sa["waves_per_simd"] == sb["waves_per_simd"], (sa, sb)
    return a, sa, moved_a


def _short_cfg(N=20, **kw):
    return make_cfg(N, solver_max_inner_iterations=60, solver_max_outer_iterations=3, **kw)


@pytest.mark.parametrize("stall", ["either", "both"])
@pytest.mark.parametrize("family", ["benchmark", "passing", "avoidance"])
def test_whole_solves_bitwise_against_the_general_form(family, stall):
    cfg = _short_cfg(solver_penalty_stall=stall)
    sc = scenes.make_family(cfg, 64, family, n_dyn=8, seed=SEEDS[family])
    _, s, _ = _assert_same_solves(cfg, sc["p"], f"{family}, {stall}")
    assert s["shape_const"] and s["axis_aligned"]


def test_full_length_solves_bitwise_against_the_general_form():
    cfg = make_cfg(20)     # the yaml's own caps
    sc = scenes.make_family(cfg, 16, "benchmark", n_dyn=8, seed=SEEDS["benchmark"])
    _assert_same_solves(cfg, sc["p"], "benchmark, the yaml's caps")


def test_long_horizon_solves_bitwise_against_the_general_form():
    cfg = make_cfg(40, solver_max_inner_iterations=30, solver_max_outer_iterations=2)     # the balanced walk of the dynamic rows
    sc = scenes.make_batch(cfg, 32, n_dyn=8, seed=78)
    _assert_same_solves(cfg, sc["p"], "N_hor = 40")


@pytest.mark.parametrize("N", [20, 40])
def test_solves_with_time_varying_shapes_bitwise_against_the_general_form(N):
    cfg = _short_cfg(N) if N == 20 else make_cfg(40, solver_max_inner_iterations=30, solver_max_outer_iterations=2)
    B = 32
    sc = scenes.make_family(cfg, B, "benchmark", n_dyn=8, seed=31)
    for b in range(B):      # every row rotated, its semi-axes changing with the step: general tables
        rows = dyn_rows(cfg, sc["p"][b])
        k = np.arange(N)
        for i in range(8):
            rows[i, :, 2] *= 1.0 + 0.01 * k
            rows[i, :, 3] *= 1.0 - 0.005 * k
            rows[i, :, 4] = 0.3 * (i + 1) + 0.02 * k
    _, s, _ = _assert_same_solves(cfg, sc["p"], f"general tables, N_hor = {N}")
    assert not s["shape_const"]


def test_solves_with_fleet_rows_bitwise_against_the_general_form():
    cfg = _short_cfg()
    sc = scenes.make_family(cfg, 64, "passing", n_dyn=8, seed=SEEDS["passing"], n_other=3)
    _, s, _ = _assert_same_solves(cfg, sc["p"], "3 fleet rows")
    assert s["max_fleet"] == 3


def test_solves_two_problems_per_wavefront_bitwise_against_the_general_form():
    cfg = _short_cfg()
    sc = scenes.make_family(cfg, 64, "benchmark", n_dyn=8, seed=SEEDS["benchmark"])
    _, s, _ = _assert_same_solves(cfg, sc["p"], "two problems per wavefront", pairing=2)
    assert s["problems_per_wavefront"] == 2


def test_promoted_solves_bitwise_against_the_general_form():
    """Every problem of a small batch is promoted once the first has finished: the promoted problems finish in the latency kernel,
    whose evaluations all go through the general form."""
    B = 48
    cfg = make_cfg(20, solver_max_inner_iterations=100, solver_max_outer_iterations=5)
    sc = scenes.make_family(cfg, B, "passing", n_dyn=8, seed=SEEDS["passing"])
    a, _, moved = _assert_same_solves(cfg, sc["p"], "tail promotion", tail_promotion=B)
    assert moved > 0
    off, _, _, _ = _solve(cfg, sc["p"])
    for f in FIELDS:
        np.testing.assert_array_equal(_bits(getattr(a, f)), _bits(getattr(off, f)), err_msg=f"promotion on / off: {f}")
