"""GPU (-m gpu): the generic-horizon kernels with static obstacles of 5 .. 8 edges against the REFERENCE's own vectors
(tests/golden/costgrad_polygons.npz, make_polygon_fixtures.py: exact boundaries, neutral rows, slot counts, magnitudes, table
forms), and what a config with wide slots runs that no other test reaches: whole solves at N_hor = 40 -- the generic solve kernel
in the stash-free carve of the compiled-horizon shape (stash_stride_c(40, 10) = 0) --, options that exist only for compiled
kernels, and the solution-level KKT check of tests/support/kkt.py at a hexagon.

Every (nstcobs, N_hor) group of the fixture runs in the table form of its cases (axis-aligned, shape-constant, general: three
instantiations of the generic cost_grad kernel), then with a spoiler problem in each more general form; psi_value -- the value-only
instantiations -- must give cost_grad's psi bit for bit on every batch."""
import numpy as np
import pytest

import oracle
from conftest import GROWING_PENALTY, make_cfg, oracle_cfg
from support import kkt, polygon_cases
from support.cost_forms import every_form
from support.edge_cases import KINDS, dyn_rows, table_kind
from test_gpu_polygon_edges import U_TOL, _same, solve_case
from test_solution_kkt import assert_kkt
from trajtrack_mpcndqn_rlboost_amd import BatchSolver, scenes
from trajtrack_mpcndqn_rlboost_amd.solver import variant_path

pytestmark = pytest.mark.gpu


# ---- 1. every fixture group against the reference, in every table form, with and without gradient
@pytest.mark.parametrize("nstcobs,N", polygon_cases.golden_groups())
def test_cost_grad_matches_reference_polygons_in_every_table_form(nstcobs, N):
    cfg = make_cfg(N, nstcobs=nstcobs)
    bs = BatchSolver(cfg)
    n = 0

    def value_only(b, form):
        r = bs.cost_grad(b["u"], b["p"], b["c"], b["y"])
        v = bs.psi_value(b["u"], b["p"], b["c"], b["y"])
        assert np.array_equal(v, r["psi"]), (form, int(np.sum(v != r["psi"])))
        v0 = bs.psi_value(b["u"], b["p"])
        assert np.array_equal(v0, bs.cost_grad(b["u"], b["p"])["psi"]), form

    print()
    for kind in KINDS:
        b = polygon_cases.golden_batch(cfg, lambda p: table_kind(cfg, p) == kind)
        worst = every_form(bs, cfg, b, kind, f"nstcobs {nstcobs} N={N}", after=value_only)
        n += len(b["idx"])
        for form, w in worst.items():
            print(f"[reference polygons: nstcobs {nstcobs}, N_hor {N}, {len(b['idx'])} {kind} cases in {form} tables] worst relative errors "
                  + ", ".join(f"{k} {v:.1e}" for k, v in w.items()))
    assert n == len(polygon_cases.golden_batch(cfg)["idx"]) > 0
    assert bs.last_shape()["problems_per_wavefront"] == 1
    bs.close()


# ---- 2. solves at N_hor = 40 with wide slots
def solve_case_40(B=32):
    """The scene of test_gpu_polygon_edges.solve_case at N_hor = 40 in slots of eight edges: one inflated regular heptagon (seven real
    rows and a neutral one) per problem at the reference path.  At this horizon the inner cap of 500 stops two thirds of the
    problems of this family whether or not an obstacle is near (the inner problem of the second outer step ends with a
    fixed-point residual of 1e-8 .. 1e-9 against its tolerance of 1e-5 x the step), so the cap is 2000 here: the oracle then
    converges on 23 of 32."""
    cfg = make_cfg(40, nstcobs=24, solver_max_inner_iterations=2000, **GROWING_PENALTY)
    sc, verts = polygon_cases.hexagon_scene(cfg, B, seed=40, nv=7)
    return cfg, sc, verts


def test_solves_around_a_heptagon_at_forty_steps_match_the_oracle():
    cfg, sc, verts = solve_case_40()
    B = len(verts)
    bs = BatchSolver(cfg, latency_batch=0)                             # the throughput kernel: one wavefront per problem ...
    res = bs.solve(sc["p"])
    assert not bs.last_shape()["latency_kernel"] and bs.last_shape()["max_static"] == 1
    team = BatchSolver(cfg)                                            # ... and what a batch of this size takes by the library's rule
    _same(res, team.solve(sc["p"]))
    assert team.last_shape()["latency_kernel"]
    team.close()
    uo, _, ro, _ = oracle.solve_batch(oracle_cfg(cfg), sc["p"])
    assert (ro["status"] == 0).sum() >= B // 2                         # the scene: the oracle alone converges on half of the batch
    both = (res.status == 0) & (ro["status"] == 0)
    du = np.max(np.abs(res.solution - uo), axis=1)
    print(f"\n[heptagon, nstcobs 24, N_hor 40] converged: GPU {int((res.status == 0).sum())}, oracle {int((ro['status'] == 0).sum())}, both "
          f"{int(both.sum())} of {B}; max |du| over those {du[both].max():.2e}; equal statuses {(res.status == ro['status']).mean():.2f}")
    assert both.sum() >= B // 4
    assert du[both].max() <= U_TOL
    assert (res.status == ro["status"]).mean() >= 0.85
    # a converged plan is feasible to delta in the polygon term restated here -- every F2_i is S, the sum over the steps of the product
    # of squared hinges (no dynamic row), so S <= ||F2|| <= delta -- and the polygon does cover the reference path of some problems
    pos = polygon_cases.rollout(sc["start"], res.solution, cfg.ts)
    off = cfg.offsets()
    crossing, deepest = 0, -np.inf
    for i in range(B):
        rows = sc["p"][i, off["os"]:off["os"] + 24]
        if res.status[i] == 0:
            h = rows[None, 0:8] - rows[None, 8:16] * pos[i][:, 0:1] - rows[None, 16:24] * pos[i][:, 1:2]
            S = float(np.sum(np.prod(np.maximum(h, 0.0) ** 2, axis=1)))
            assert S <= cfg.solver_delta_tolerance * (1 + 1e-9), (i, S)
            deepest = max(deepest, float(h.min(axis=1).max()))
        crossing += polygon_cases.smallest_halfplane_value(rows, 8, sc["ref"][i, :, :2]).max() > 1e-3
    print(f"[heptagon, nstcobs 24, N_hor 40] the deepest converged plan is {deepest:.1e} (half-plane units) inside; the heptagon covers "
          f"the reference path of {crossing} problems")
    assert crossing >= B // 8
    bs.close()


# ---- 4. options that exist only for the kernels with a compiled horizon
def options_case(N, B=16):
    """padded quads (walls, box) and hexagons side by side, straight-moving axis-aligned discs of constant shape: the tables the
    linear form of the N_hor = 40 variant build would take, were the horizon compiled"""
    cfg = make_cfg(N, nstcobs=18)
    sc = scenes.make_family(cfg, B, "passing", n_dyn=3, seed=400 + N)
    hx, _ = polygon_cases.hexagon_scene(cfg, B, seed=401 + N, n_dyn=3, dyn_clearance=0.1, with_walls=True, on_track=False,
                                        v_init_range=(0.0, 1.2))
    p = np.where((np.arange(B) % 2 == 0)[:, None], sc["p"], hx["p"])
    for i in range(B):
        rows = dyn_rows(cfg, p[i])                          # a view into p
        for r in (rows[j] for j in np.nonzero(np.any(rows != 0.0, axis=(1, 2)))[0]):
            vel = r[1, 0:2] - r[0, 0:2]
            r[:, 0:2] = r[0, 0:2] + np.arange(N)[:, None] * vel
            r[:, 2:6] = [r[0, 2], r[0, 3], 0.0, r[0, 5]]
        assert table_kind(cfg, p[i]) == "axis"
    rng = np.random.default_rng(N)
    u = np.stack([rng.uniform(-0.7, 1.8, (B, N)), rng.uniform(-0.7, 0.7, (B, N))], axis=2).reshape(B, 2 * N)
    return cfg, p, u, rng.choice([0.0, 10.0, 250.0], B), rng.uniform(-3, 3, (B, 2 * N))


@pytest.mark.parametrize("option", ["pairing=2", "linear40"])
def test_options_of_the_compiled_kernels_are_accepted_and_change_nothing_with_wide_slots(option):
    N = 20 if option == "pairing=2" else 40
    cfg, p, u, c, y = options_case(N)
    plain = BatchSolver(cfg)
    other = BatchSolver(cfg, pairing=2) if option == "pairing=2" else BatchSolver(cfg, library=variant_path("linear40"))
    for latency_batch in (None, 0):                       # the latency kernel (B = 16 is below its limit), then the throughput kernel
        if latency_batch is not None:
            plain.close(); other.close()
            plain = BatchSolver(cfg, latency_batch=0)
            other = (BatchSolver(cfg, pairing=2, latency_batch=0) if option == "pairing=2"
                     else BatchSolver(cfg, library=variant_path("linear40"), latency_batch=0))
        a, b = plain.solve(p), other.solve(p)
        s = other.last_shape()
        assert not (s["latency_kernel"] and latency_batch == 0), s
        assert s["problems_per_wavefront"] == 1 and not s["linear"], s
        _same(a, b)
    ra, rb = plain.cost_grad(u, p, c, y), other.cost_grad(u, p, c, y)
    s = other.last_shape()
    assert s["problems_per_wavefront"] == 1 and not s["linear"] and s["axis_aligned"], s
    for k in ("f", "psi", "grad", "F1", "F2"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(plain.psi_value(u, p, c, y), other.psi_value(u, p, c, y))
    assert (ra["F2"][:, -1] > 0).sum() >= 2                 # some rollouts enter a polygon
    plain.close(); other.close()


# ---- 5. the solution-level check at a hexagon
def test_converged_gpu_solutions_beside_a_hexagon_are_local_minima_of_the_reference_problem():
    """tests/test_gpu_solution_kkt.py's check, with its thresholds, on every converged problem of the hexagon scene (nstcobs = 18):
    the hard constraint of a polygon is the smallest of SIX half-plane values there (tests/support/kkt.py reads the slot width from
    the config)."""
    cfg, sc, verts = solve_case()
    ocfg = oracle_cfg(cfg)
    bs = BatchSolver(cfg)
    res = bs.solve(sc["p"])
    bs.close()
    conv = np.where(res.status == 0)[0]
    assert len(conv) >= len(verts) // 2, len(conv)
    worst = dict(pg_residual=0.0, scipy_move=0.0, scipy_f_gain_rel=-1.0, g_static_max=-np.inf)
    for i in conv:
        r = kkt.check_solution(cfg, ocfg, sc["p"][i], res.solution[i], res.lagrange_multipliers[i])
        assert_kkt(r, f"hexagon problem {i}")
        for k in worst:
            worst[k] = max(worst[k], r[k])
    assert worst["g_static_max"] > -0.1                      # some converged plan passes the hexagon within a tenth (half-plane units)
    print(f"\n[kkt, hexagon, nstcobs 18] {len(conv)} converged solves checked; worst {worst}")
