"""CPU: the oracle (oracle/mpc_oracle.c) against the edge-case vectors generated from the reference's own source
(tests/golden/make_edge_fixtures.py): exact ties of the path minimum, hairpins, table forms, horizons 2-64, boundaries and
large coordinates.  The oracle is the yardstick of the whole GPU suite, so it has to hold here first."""
import numpy as np
import pytest

import oracle
from conftest import load_golden, make_cfg, oracle_cfg
from support.edge_cases import KINDS, dyn_rows, table_kind

RTOL = 1e-11  # the norm of tests/test_oracle_golden.py


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def edge_cases(family=None):
    """(index, N, u, p, c, y) of every case of costgrad_edges.npz (of one family), unpadded"""
    fx = load_golden("costgrad_edges.npz")
    for i in range(len(fx["N"])):
        if family is not None and str(fx["family"][i]) != family:
            continue
        N = int(fx["N"][i])
        n_p = make_cfg(N).num_params
        yield i, N, fx["u"][i, :2 * N], fx["p"][i, :n_p], float(fx["c"][i]), fx["y"][i, :2 * N]


def _nearest(P, s1, s2):
    """d^2 and nearest point of segment (s1, s2) seen from P, the reference's formula (mpc_generator.py:28-36)"""
    d = s2 - s1
    t = min(max(np.dot(P - s1, d) / (d[0] ** 2 + d[1] ** 2 + 1e-16), 0.0), 1.0)
    q = s1 + t * d
    return float(np.sum((q - P) ** 2)), q


def test_edge_fixtures_cover_every_family_and_horizon():
    fx = load_golden("costgrad_edges.npz")
    assert sorted(set(fx["family"].tolist())) == ["A", "B", "C", "D", "E", "F"]
    assert {2, 12, 20, 33, 40, 64} <= set(fx["N"].tolist())
    # family A really holds exact ties of the path minimum (u = 0: every predicted position is p[0:2]) whose tying segments
    # have DIFFERENT nearest points -- the gradient depends on which one wins -- next to ties at a shared vertex (same point)
    distinct = shared = 0
    for i, N, u, p, c, y in edge_cases("A"):
        assert not np.any(u)
        r0 = make_cfg(N).offsets()["r"]
        V = p[r0:r0 + 3 * N].reshape(N, 3)[:, :2]
        P = p[0:2]
        kinds = set()
        for k in range(N):
            hits = [_nearest(P, V[j], V[min(j + 1, N - 1)]) for j in range(k, N)]
            m = min(h[0] for h in hits)
            pts = {tuple(h[1]) for h in hits if h[0] == m}
            if sum(h[0] == m for h in hits) >= 2:
                kinds.add("distinct" if len(pts) >= 2 else "shared")
        distinct += "distinct" in kinds
        shared += kinds == {"shared"}
    assert distinct >= 20 and shared >= 3, (distinct, shared)


def test_every_table_form_has_cases_whose_ellipses_matter():
    """Each table form (tests/test_gpu_cost_edges.py runs every kind as a batch of its own) is pinned at a compiled and at a
    runtime horizon by cases whose dynamic rows change the reference's f: without them the form would go unchecked."""
    fx = load_golden("costgrad_edges.npz")
    seen = set()
    for i, N, u, p, c, y in edge_cases():
        cfg = make_cfg(N)
        q = p.copy()
        dyn_rows(cfg, q)[:] = 0.0
        if oracle.cost_grad(oracle_cfg(cfg), u, q)["f"] != fx["f"][i]:
            seen.add((table_kind(cfg, p), N in (20, 40)))
    assert seen == {(k, compiled) for k in KINDS for compiled in (True, False)}, seen


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E", "F"])
def test_oracle_matches_reference_edge_fixtures(family):
    fx = load_golden("costgrad_edges.npz")
    n = 0
    for i, N, u, p, c, y in edge_cases(family):
        cfg = oracle_cfg(make_cfg(N))
        assert p.size == oracle.num_params(cfg)
        r = oracle.cost_grad(cfg, u, p, c, y)
        r0 = oracle.cost_grad(cfg, u, p, 0.0, None)
        tag = str(fx["tag"][i])
        assert _rel(r["f"], fx["f"][i]) < RTOL, tag
        assert _rel(r["psi"], fx["psi"][i]) < RTOL, tag
        assert _rel(r["grad"], fx["grad_psi"][i, :2 * N]) < RTOL, tag
        assert _rel(r0["grad"], fx["grad_f"][i, :2 * N]) < RTOL, tag
        assert _rel(r["F1"], fx["F1"][i, :2 * N]) < RTOL, tag
        assert _rel(r["F2"], fx["F2"][i]) < RTOL, tag
        n += 1
    assert n > 0
