"""CPU: the oracle's polygon term with 5 .. 8 edges (oracle/mpc_oracle.c, the loop over the edges) against vectors generated from
the reference's own source (tests/golden/make_polygon_fixtures.py -> costgrad_polygons.npz): points exactly on edges and
vertices, neutral rows at the end and in the middle of a slot, 1 .. Nstcobs slots in use at every width, products of 1e7 and of
1e-48, large coordinates, every table form.  The oracle is the yardstick of tests/test_gpu_polygon_edges.py and
tests/test_gpu_polygon_golden.py, so it has to hold here first."""
import numpy as np
import pytest

import oracle
from conftest import make_cfg, oracle_cfg
from support import polygon_cases
from support.edge_cases import KINDS, table_kind

RTOL = 1e-11  # the norm of tests/test_oracle_golden.py and tests/test_oracle_edges.py
FAMILIES = ["P", "Q", "R", "S", "T"]


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def polygon_cases_of(family=None):
    """(index, cfg, u, p, c, y) of every case of costgrad_polygons.npz (of one family), unpadded"""
    fx = polygon_cases.golden()
    for i in range(len(fx["N"])):
        if family is not None and str(fx["family"][i]) != family:
            continue
        N = int(fx["N"][i])
        cfg = make_cfg(N, nstcobs=int(fx["nstcobs"][i]))
        yield i, cfg, fx["u"][i, :2 * N], fx["p"][i, :cfg.num_params], float(fx["c"][i]), fx["y"][i, :2 * N]


def test_polygon_fixtures_cover_every_width_horizon_and_table_form():
    fx = polygon_cases.golden()
    assert sorted(set(fx["family"].tolist())) == FAMILIES
    groups = set(polygon_cases.golden_groups())
    assert {(w, N) for w in (15, 18, 21, 24) for N in (12, 20, 40)} <= groups and {2, 33} <= {N for _, N in groups}
    # every generic cost_grad instantiation (three table forms) has cases of its own at a compiled-horizon shape and at a runtime one
    seen = {(table_kind(cfg, p), cfg.N_hor in (20, 40)) for i, cfg, u, p, c, y in polygon_cases_of()}
    assert seen == {(k, compiled) for k in KINDS for compiled in (True, False)}, seen
    # slot counts at the odd widths: an odd number of doubles in front of the next even offset
    used = {(int(cfg.nstcobs), polygon_cases.halfplane_values(cfg, p, u).shape[1]) for i, cfg, u, p, c, y in polygon_cases_of("R")}
    assert {(w, n) for w in (15, 21) for n in (1, 2, 3, 5, 10)} <= used, used


def test_polygon_fixtures_hold_inside_outside_and_exact_boundaries_in_every_family():
    """Per family: cases whose rollout enters a polygon (S > 0), cases that stay out (S = 0), cases with a half-plane value that
    is exactly 0 at some step.  S is the reference's F2 of a dynamic row that is not in use (F2_i = S + D_i, D_i = 0)."""
    fx = polygon_cases.golden()
    print()
    for family in FAMILIES:
        n_in = n_out = n_zero = n_two = 0
        for i, cfg, u, p, c, y in polygon_cases_of(family):
            S = fx["F2"][i][-1]
            h = polygon_cases.halfplane_values(cfg, p, u)
            n_in += S > 0.0
            n_out += S == 0.0
            n_zero += bool(np.any(h == 0.0))
            n_two += bool(np.any(np.sum(np.all(h > 0.0, axis=2), axis=1) >= 2))
        print(f"[polygon fixtures] family {family}: S > 0 in {n_in}, S = 0 in {n_out}, a half-plane value exactly 0 in {n_zero}, "
              f"a step inside two polygons in {n_two}")
        if family in "PQR":
            assert n_in > 0 and n_out > 0 and n_zero > 0, family
        if family == "R":
            assert n_two > 0


def test_neutral_rows_in_the_middle_of_a_slot_change_nothing_in_the_reference():
    fx = polygon_cases.golden()
    tags = fx["tag"].tolist()
    pairs = [(i, i + 1) for i, t in enumerate(tags[:-1]) if t.startswith("hull of") and t.endswith("at the end")]
    assert len(pairs) >= 8
    for i, j in pairs:
        assert tags[j] == tags[i].replace("at the end", "at the middle")
        assert fx["psi"][i] == fx["psi"][j] and np.array_equal(fx["F2"][i], fx["F2"][j]) and fx["F2"][i].min() > 0.0


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_matches_reference_polygon_fixtures(family):
    fx = polygon_cases.golden()
    n = 0
    worst = dict(f=0.0, psi=0.0, grad=0.0, grad_f=0.0, F1=0.0, F2=0.0, psi0=0.0)
    for i, cfg, u, p, c, y in polygon_cases_of(family):
        N = int(cfg.N_hor)
        ocfg = oracle_cfg(cfg)
        assert p.size == oracle.num_params(ocfg)
        r = oracle.cost_grad(ocfg, u, p, c, y)
        r0 = oracle.cost_grad(ocfg, u, p, 0.0, None)          # c = 0: psi is f, the gradient is grad f
        tag = str(fx["tag"][i])
        errs = dict(f=_rel(r["f"], fx["f"][i]), psi=_rel(r["psi"], fx["psi"][i]), grad=_rel(r["grad"], fx["grad_psi"][i, :2 * N]),
                    grad_f=_rel(r0["grad"], fx["grad_f"][i, :2 * N]), F1=_rel(r["F1"], fx["F1"][i, :2 * N]),
                    F2=_rel(r["F2"], fx["F2"][i]), psi0=_rel(r0["psi"], fx["f"][i]))
        for k, v in errs.items():
            worst[k] = max(worst[k], v)
            assert v < RTOL, (tag, k, v)
        n += 1
    print(f"\n[oracle vs reference, family {family}] {n} cases, worst relative errors {worst}")
    assert n > 0
