#!/usr/bin/env python3
"""Golden vectors of the cost / gradient path with static obstacles of 5 to 8 edges (nstcobs = 15, 18, 21, 24), FROM THE
REFERENCE ITSELF.

Run in the build container only (needs /root/reference, like make_fixtures.py, whose CasADi / opengen stand-ins and
``evaluate`` it imports; scene pieces come from make_edge_fixtures.py):

    python tests/golden/make_polygon_fixtures.py

costgrad_polygons.npz holds one record per case, padded to the largest shape: ``N``, ``nstcobs``, ``family`` (P..T),
``tag``, ``u [C, 2 Nmax]``, ``p [C, np(Nmax, 24)]``, ``c``, ``y`` and the reference's ``f, grad_f, F1, F2, psi,
grad_psi``.  Row i uses the first 2 N[i] entries of u / y / grad / F1 and the first np(N[i], nstcobs[i]) of p.
A static slot is b[ne] | a0[ne] | a1[ne], ne = nstcobs / 3; a point is inside where every b - a0 x - a1 y > 0.

Families:
  P  exact boundaries.  u = 0 and a standing robot: every predicted position IS p[0:2].  Half-planes with dyadic
     coefficients: the point on one edge, on a vertex (two values exactly 0), one ulp inside and one ulp outside an
     edge, at the centre, and strictly inside one slot while on an edge of a second one.  Then moving rollouts one step
     of which lies 5e-10 inside / outside an edge of a regular hull.
  Q  neutral rows (1, 0, 0): hulls of 3 .. ne - 1 edges crossed by the rollout, each twice -- padded at the end, as the
     feeders pad, and with the neutral rows in the middle.  The reference's values of the two are equal (asserted).
     A dyadic triangle with the standing robot on one of its edges, in both layouts.
  R  1, 2, 3, 5 and all Nstcobs slots in use; full and padded hulls side by side; some step inside two overlapping
     polygons at once (asserted); a standing robot inside one dyadic slot and on an edge of the next, and on an edge only.
  S  magnitudes: every half-plane value 2 .. 3 (product around 1e6 at eight edges) and around 1e-3 (1e-48); polygons and
     path 200 .. 500 m from the origin; c in {0, 1, 1e6}, |y| up to 1e3.
  T  one R geometry per width with dynamic rows of each kind of tests/support/edge_cases.py (axis, rot, var).
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (registers the stand-ins and imports the reference)
import make_edge_fixtures as mef  # noqa: E402  (scene pieces; nothing of it runs on import)

OUT = os.path.join(HERE, "costgrad_polygons.npz")
WIDTHS = (15, 18, 21, 24)
HORIZONS = (20, 40, 12)
NEUTRAL = (1.0, 0.0, 0.0)
_cfgs: dict = {}


def cfg_of(N, nstcobs):
    if (N, nstcobs) not in _cfgs:
        src = open(os.path.join(mf.REF, "config", "mpc_default.yaml")).read()
        assert "N_hor: 20" in src and "nstcobs: 12" in src
        src = src.replace("N_hor: 20", f"N_hor: {N}").replace("nstcobs: 12", f"nstcobs: {nstcobs}")
        with tempfile.NamedTemporaryFile("w", suffix=".yaml", delete=False) as fh:
            fh.write(src)
            path = fh.name
        cfg = mf.Configurator(path, verbose=False)
        os.unlink(path)
        assert cfg.N_hor == N and cfg.nstcobs == nstcobs
        _cfgs[(N, nstcobs)] = cfg
    return _cfgs[(N, nstcobs)]


def horizon(j, w):
    """the horizons go round with the case number, shifted by the width: every (width, horizon) pair gets cases"""
    return HORIZONS[(j + WIDTHS.index(w)) % 3]


# --------------------------------------------------------------------------------------------
# slots
# --------------------------------------------------------------------------------------------
def set_slot(cfg, p, o, rows, layout="end"):
    """rows: list of (b, a0, a1), at most ne; neutral rows fill the slot at its end or after the first real row"""
    ne = cfg.nstcobs // 3
    pad = [NEUTRAL] * (ne - len(rows))
    rows = list(rows) + pad if layout == "end" else list(rows[:1]) + pad + list(rows[1:])
    assert len(rows) == ne
    os0 = mf.offsets(cfg)[2]
    p[os0 + o * 3 * ne:os0 + (o + 1) * 3 * ne] = [r[0] for r in rows] + [r[1] for r in rows] + [r[2] for r in rows]


def hull_rows(verts):
    """(b, a0, a1) per edge of a convex polygon given by ordered vertices, normalised like the reference's facet
    enumeration (a . (v - centre) = 1 on every facet, b = a . centre + 1; util/utils_geo.py)"""
    v = np.asarray(verts, float)
    c = v.mean(axis=0)
    rows = []
    for e in range(len(v)):
        d = v[(e + 1) % len(v)] - v[e]
        n = np.array([d[1], -d[0]])
        a = n / np.dot(n, v[e] - c)
        rows.append((float(np.dot(a, c) + 1.0), float(a[0]), float(a[1])))
    return rows


def polygon(rng, centre, nv, radius, regular=True, phase=None):
    gaps = np.ones(nv) if regular else rng.uniform(0.7, 1.3, nv)
    ang = (rng.uniform(0, 2 * np.pi) if phase is None else phase) + 2 * np.pi * np.cumsum(gaps) / gaps.sum()
    return np.asarray(centre, float) + radius * np.stack([np.cos(ang), np.sin(ang)], axis=-1)


# dyadic half-planes around (8, 4): x < 10, x > 6, y < 6, y > 2, then cuts through the corners x + y < 15, x - y < 7,
# y - x < -1, x + y > 9 -- every vertex has dyadic coordinates: (10, 5) lies on rows 0 and 4, both values exactly 0
EXACT = [(5.0, 0.5, 0.0), (-3.0, -0.5, 0.0), (3.0, 0.0, 0.5), (-1.0, 0.0, -0.5),
         (3.75, 0.25, 0.25), (1.75, 0.25, -0.25), (-0.25, -0.25, 0.25), (-2.25, -0.25, -0.25)]


def exact_rows(n, shift=(0.0, 0.0)):
    return [(b + a0 * shift[0] + a1 * shift[1], a0, a1) for b, a0, a1 in EXACT[:n]]


def values(rows, pt):
    return np.array([b - a0 * pt[0] - a1 * pt[1] for b, a0, a1 in rows])


# --------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------
def rollout(cfg, p, u):
    s = np.array(p[0:3], float)
    out = []
    for k in range(cfg.N_hor):
        s = np.asarray(mf.unicycle_model(s, np.asarray(u[2 * k:2 * k + 2], float), cfg.ts), float)
        out.append(s[:2].copy())
    return np.array(out)


def standing(cfg, x, y, rng, n_dyn=0):
    """u = 0, the robot at (x, y); a path beside it, n_dyn axis-aligned rows near it"""
    N = cfg.N_hor
    p = mef.base_p(cfg, x, y, 0.5, 0.0, 0.0)
    mef.set_path(cfg, p, [np.array([x + 0.25 * (k + 1), y + 0.5]) for k in range(N)])
    if n_dyn:
        mef.add_obstacles(cfg, p, rng, np.array([x, y]), 1.5, n_dyn=n_dyn, n_stc=0, n_other=1, kinds=("axis",))
    return np.zeros(2 * N), p


def moving(cfg, rng, kinds=("rot",), origin=(0.0, 0.0), n_other=1):
    """a random path near the robot, random inputs that drive forward, dynamic rows of the given kinds; returns u, p and
    the predicted positions [N, 2]"""
    N = cfg.N_hor
    o = np.array(origin, float)
    P = o + rng.uniform(-2, 2, 2)
    th = rng.uniform(-np.pi, np.pi)
    pts, hs = mef.curve(rng, P, th, N, step=(0.2, 0.3))
    p = mef.base_p(cfg, P[0], P[1], th, rng.uniform(0.3, 1.2), rng.uniform(-0.3, 0.3))
    mef.set_path(cfg, p, pts, hs)
    mef.add_obstacles(cfg, p, rng, pts[N // 3], 1.0, n_dyn=len(kinds), n_stc=0, n_other=n_other, kinds=kinds or ("rot",))
    v = rng.uniform(0.3, 1.5, N)
    w = rng.uniform(-0.5, 0.5, N)
    u = np.stack([v, w], axis=1).reshape(-1)
    return u, p, rollout(cfg, p, u)


def smallest(rows, pos):
    return np.array([values(rows, q).min() for q in pos])


# --------------------------------------------------------------------------------------------
# families
# --------------------------------------------------------------------------------------------
def family_P(rng):
    cases = []
    inside, outside = np.nextafter(10.0, 0.0), np.nextafter(10.0, 20.0)
    spots = [("on an edge", (10.0, 4.0), None), ("on a vertex (two values exactly 0)", (10.0, 5.0), None),
             ("one ulp inside an edge", (inside, 4.0), None), ("one ulp outside an edge", (outside, 4.0), None),
             ("at the centre", (8.0, 4.0), None),
             ("strictly inside slot 0, on an edge of slot 1", (8.5, 4.0), (2.5, 0.0))]
    j = 0
    for w in WIDTHS:
        ne = w // 3
        for what, pt, second in spots:
            cfg = cfg_of(horizon(j, w), w)
            u, p = standing(cfg, pt[0], pt[1], rng, n_dyn=j % 3)
            rows = exact_rows(ne)
            set_slot(cfg, p, 0, rows)
            h = values(rows, pt)
            if second is not None:
                rows2 = exact_rows(ne, second)
                set_slot(cfg, p, 1, rows2)
                assert h.min() > 0 and values(rows2, pt)[1] == 0.0 and np.sum(values(rows2, pt) == 0.0) == 1
            elif "vertex" in what:
                assert h[0] == 0.0 and h[4] == 0.0 and np.sum(h == 0.0) == 2 and h.min() == 0.0
            elif "on an edge" in what:
                assert h[0] == 0.0 and np.sum(h == 0.0) == 1 and h.min() == 0.0
            elif "inside" in what:
                assert 0.0 < h[0] < 1e-15 and h.min() == h[0]
            elif "outside" in what:
                assert -1e-15 < h[0] < 0.0
            c = (0.0, 10.0, 250.0)[j % 3]
            cases.append((cfg, "P", f"standing robot {what}, {ne} edges", u, p, c, np.zeros(u.size)))
            j += 1
        for side in (1.0, -1.0):           # a step of a moving rollout 5e-10 (in half-plane units) inside / outside edge 0
            cfg = cfg_of(horizon(j, w), w)
            u, p, pos = moving(cfg, rng, kinds=("rot",) * (j % 2))
            k = int(rng.integers(cfg.N_hor // 2, cfg.N_hor))
            r = rng.uniform(0.8, 1.4)
            phase = rng.uniform(0, 2 * np.pi)
            v = polygon(rng, (0.0, 0.0), ne, r, phase=phase)
            mid = 0.5 * (v[0] + v[1])                                    # the middle of edge 0; the centre is the origin
            rows = hull_rows(v + (pos[k] - mid * (1.0 - side * 5e-10)))  # value of row 0 at pos[k]: side * 5e-10
            h = values(rows, pos[k])
            assert 1e-10 < side * h[0] < 1e-9 and np.all(h[1:] > 1e-3), h
            set_slot(cfg, p, 0, rows)
            cases.append((cfg, "P", f"moving: step {k} is {abs(h[0]):.1e} {'inside' if side > 0 else 'outside'} an edge, {ne} edges",
                          u, p, 10.0, np.zeros(u.size)))
            j += 1
    return cases


def family_Q(rng):
    cases = []
    j = 0
    for w in WIDTHS:
        ne = w // 3
        for nv in sorted({3, ne - 1}):
            cfg = cfg_of(horizon(j, w), w)
            u, p, pos = moving(cfg, rng, kinds=("rot", "axis")[:j % 3])
            k = int(rng.integers(cfg.N_hor // 3, cfg.N_hor))
            rows = hull_rows(polygon(rng, pos[k] + rng.uniform(-0.1, 0.1, 2), nv, rng.uniform(0.7, 1.3), regular=bool(j % 2)))
            assert smallest(rows, pos).max() > 0.05                        # the rollout crosses the hull
            c, y = float(rng.choice([10.0, 250.0])), rng.uniform(-3, 3, u.size) * (j % 2 == 0)
            pair = []
            for layout in ("end", "middle"):
                q = p.copy()
                set_slot(cfg, q, 0, rows, layout)
                pair.append((cfg, "Q", f"hull of {nv} edges in a slot of {ne}, neutral rows at the {layout}", u, q, c, y))
            cases += pair
            j += 1
    # the standing robot on an edge of a dyadic triangle x < 10, y > 2, y - x < -1 (rows 0, 3, 6 of EXACT)
    tri = [EXACT[0], EXACT[3], EXACT[6]]
    for w, layout, pt in ((15, "end", (10.0, 4.0)), (21, "middle", (10.0, 4.0)), (18, "end", (9.0, 4.0)), (24, "middle", (9.0, 4.0))):
        cfg = cfg_of(20 if w in (15, 24) else 40, w)
        u, p = standing(cfg, pt[0], pt[1], rng, n_dyn=1)
        set_slot(cfg, p, 0, tri, layout)
        h = values(tri, pt)
        assert (h.min() == 0.0 and np.sum(h == 0.0) == 1) if pt[0] == 10.0 else h.min() > 0.0
        cases.append((cfg, "Q", f"standing robot {'on an edge of' if pt[0] == 10.0 else 'inside'} a dyadic triangle in a slot of "
                      f"{w // 3}, neutral rows at the {layout}", u, p, 10.0, np.zeros(u.size)))
    return cases


def slots_scene(cfg, rng, n_slots, kinds, origin=(0.0, 0.0)):
    """n_slots hulls: slots 0 and 1 overlap on a rollout point (a full hull and a padded one), the others stand on or beside
    later rollout points; full and padded hulls alternate"""
    ne = cfg.nstcobs // 3
    u, p, pos = moving(cfg, rng, kinds=kinds, origin=origin)
    N = cfg.N_hor
    k = int(rng.integers(N // 3, N))
    inside = np.zeros(N, int)
    for o in range(n_slots):
        nv = ne if o % 2 == 0 else int(rng.integers(3, ne))
        if o < 2:
            centre = pos[k] + rng.uniform(-0.1, 0.1, 2)
        else:
            centre = pos[int(rng.integers(0, N))] + rng.uniform(-2.5, 2.5, 2)
        rows = hull_rows(polygon(rng, centre, nv, rng.uniform(0.6, 1.2), regular=bool(rng.integers(0, 2))))
        set_slot(cfg, p, o, rows, "end" if o % 4 < 2 else "middle")
        inside += smallest(rows, pos) > 0.0
    return u, p, pos, inside


def family_R(rng):
    cases = []
    j = 0
    for w in WIDTHS:
        ne = w // 3
        Ns = cfg_of(20, w).Nstcobs
        for n_slots in ((1, 2, 3, 5, Ns) if w in (15, 21) else (3, Ns)):
            cfg = cfg_of(horizon(j, w), w)
            u, p, pos, inside = slots_scene(cfg, rng, n_slots, ("rot", "axis")[:j % 3])
            assert inside.max() >= min(n_slots, 2), (w, n_slots, inside)    # some step is inside two polygons at once
            cases.append((cfg, "R", f"{n_slots} of {Ns} slots in use, {ne} edges, up to {inside.max()} polygons around one step",
                          u, p, float(rng.choice([10.0, 250.0, 6250.0])), rng.uniform(-3, 3, u.size)))
            j += 1
    # exact boundaries with several slots: inside slot 0 and on an edge of slot 2 (S > 0); on an edge of slot 1 only (S = 0)
    for w in (15, 21):
        ne = w // 3
        for what, pt in (("inside slot 0, on an edge of slot 2", (8.5, 4.0)), ("on an edge of slot 1, outside the others", (14.5, 4.0))):
            cfg = cfg_of(horizon(j, w), w)
            u, p = standing(cfg, pt[0], pt[1], rng, n_dyn=2)
            sl = [exact_rows(ne), exact_rows(ne - 1, (4.5, 0.0)), exact_rows(ne, (2.5, 0.0))]
            for o, rows in enumerate(sl):
                set_slot(cfg, p, o, rows, "middle" if o == 1 else "end")
            hs = [values(rows, pt) for rows in sl]
            if pt[0] == 8.5:
                assert hs[0].min() > 0.0 and hs[2][1] == 0.0 and hs[1].min() < 0.0
            else:
                assert hs[1][0] == 0.0 and hs[1].min() == 0.0 and hs[0].min() < 0.0 and hs[2].min() < 0.0
            cases.append((cfg, "R", f"standing robot {what}, 3 slots, {ne} edges", u, p, 10.0, np.zeros(u.size)))
            j += 1
    # the odd horizons, once each
    for N, w in ((2, 15), (33, 21)):
        cfg = cfg_of(N, w)
        u, p, pos = moving(cfg, rng, kinds=("rot",))
        rows = hull_rows(polygon(rng, pos[-1] + rng.uniform(-0.05, 0.05, 2), w // 3, 1.0))
        set_slot(cfg, p, 0, rows)
        set_slot(cfg, p, 1, hull_rows(polygon(rng, pos[0] + rng.uniform(-0.05, 0.05, 2), 3, 0.9)))
        assert smallest(rows, pos).max() > 0.05
        cases.append((cfg, "R", f"horizon {N}: 2 slots, {w // 3} edges", u, p, 10.0, rng.uniform(-3, 3, u.size)))
    return cases


def magnitude_rows(rng, ne, pt, lo, hi):
    """ne half-planes with unit normals around the compass whose values at pt are drawn from [lo, hi]"""
    ang = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(ne) / ne
    rows = []
    for a in ang:
        a0, a1 = float(np.cos(a)), float(np.sin(a))
        rows.append((a0 * pt[0] + a1 * pt[1] + rng.uniform(lo, hi), a0, a1))
    return rows


def family_S(rng):
    cases = []
    j = 0
    for w in (24, 15):
        ne = w // 3
        for what, lo, hi in (("2 .. 3", 2.0, 3.0), ("around 1e-3", 0.5e-3, 2e-3)):
            for move in (False, True):
                cfg = cfg_of(horizon(j, w), w)
                if move:
                    u, p, pos = moving(cfg, rng, kinds=("rot",))
                    pt = pos[int(rng.integers(cfg.N_hor // 2, cfg.N_hor))]
                    y = rng.uniform(-3, 3, u.size)
                else:
                    pt = rng.uniform(-4, 4, 2)
                    u, p = standing(cfg, pt[0], pt[1], rng, n_dyn=1)
                    y = np.zeros(u.size)
                rows = magnitude_rows(rng, ne, pt, lo, hi)
                h = values(rows, pt)
                assert lo * 0.99 < h.min() and h.max() < hi * 1.01
                set_slot(cfg, p, 0, rows)
                cases.append((cfg, "S", f"{'a step of a moving rollout' if move else 'standing robot'} with every half-plane value {what}, "
                              f"{ne} edges: product {np.prod(h * h):.1e}", u, p, 10.0, y))
                j += 1
    for w in WIDTHS:                       # large coordinates
        cfg = cfg_of(horizon(j, w), w)
        r, a = rng.uniform(200.0, 500.0), rng.uniform(-np.pi, np.pi)
        u, p, pos, inside = slots_scene(cfg, rng, 3, ("rot",), origin=(r * np.cos(a), r * np.sin(a)))
        assert inside.max() >= 2
        cases.append((cfg, "S", f"large coordinates |x|~{r:.0f} m, {w // 3} edges", u, p, 10.0, rng.uniform(-3, 3, u.size)))
        j += 1
    for c, ys, w in ((0.0, 0.0, 18), (1.0, 1e3, 21), (1e6, 0.0, 24), (1e6, 1e3, 15)):
        cfg = cfg_of(horizon(j, w), w)
        u, p, pos, inside = slots_scene(cfg, rng, 2, ("axis",))
        assert inside.max() >= 2
        y = np.linspace(-ys, ys, u.size)
        cases.append((cfg, "S", f"c={c:g} |y|<={ys:g}, {w // 3} edges", u, p, c, y))
        j += 1
    return cases


def family_T(rng):
    cases = []
    j = 0
    for w in WIDTHS:
        for N in HORIZONS:
            kind = ("axis", "rot", "var")[(j + j // 3) % 3]           # every width and every horizon meets every kind
            cfg = cfg_of(N, w)
            kinds = dict(axis=("axis", "axis"), rot=("rot", "axis", "rot"), var=("var", "rot", "axis"))[kind]
            u, p, pos, inside = slots_scene(cfg, rng, 3, kinds)
            assert inside.max() >= 2
            cases.append((cfg, "T", f"{kind} tables, 3 slots, {w // 3} edges", u, p, float(rng.choice([10.0, 250.0])),
                          np.zeros(u.size)))
            j += 1
    return cases


# --------------------------------------------------------------------------------------------
def main():
    rng = np.random.default_rng(20261019)
    cases = family_P(rng) + family_Q(rng) + family_R(rng) + family_S(rng) + family_T(rng)
    Nmax = max(cs[0].N_hor for cs in cases)
    npmax = mf.np_of(cfg_of(Nmax, max(WIDTHS)))
    C = len(cases)
    n2 = cfg_of(20, 15).Ndynobs
    U = np.zeros((C, 2 * Nmax)); Pp = np.zeros((C, npmax)); Y = np.zeros((C, 2 * Nmax)); Cc = np.zeros(C)
    f = np.zeros(C); psi = np.zeros(C); gf = np.zeros((C, 2 * Nmax)); gp = np.zeros((C, 2 * Nmax))
    F1 = np.zeros((C, 2 * Nmax)); F2 = np.zeros((C, n2))
    Ns = np.zeros(C, np.int32); Ws = np.zeros(C, np.int32)
    fam, tag = [], []
    for i, (cfg, fm, tg, u, p, c, y) in enumerate(cases):
        N = cfg.N_hor
        assert p.size == mf.np_of(cfg) and u.size == y.size == 2 * N
        r = mf.evaluate(cfg, u, p, c, y)
        assert np.all(np.isfinite(r["grad_psi"])) and np.isfinite(r["psi"]), tg
        Ns[i] = N; Ws[i] = cfg.nstcobs; U[i, :2 * N] = u; Pp[i, :p.size] = p; Y[i, :2 * N] = y; Cc[i] = c
        f[i] = r["f"]; psi[i] = r["psi"]
        gf[i, :2 * N] = r["grad_f"]; gp[i, :2 * N] = r["grad_psi"]
        F1[i, :2 * N] = r["F1"]; F2[i] = r["F2"]
        fam.append(fm); tag.append(tg)
    # family Q: the two layouts of a hull have the same values in the reference (a neutral row multiplies by exactly 1)
    for i in range(C - 1):
        if fam[i] == "Q" and tag[i].endswith("at the end") and tag[i].startswith("hull"):
            assert tag[i + 1].endswith("at the middle")
            assert psi[i] == psi[i + 1] and np.array_equal(F2[i], F2[i + 1]) and f[i] == f[i + 1], tag[i]
            assert np.max(np.abs(gp[i] - gp[i + 1])) <= 1e-13 * max(1.0, np.max(np.abs(gp[i]))), tag[i]
            assert F2[i].min() > 0.0, tag[i]
    mef.savez_deterministic(OUT, N=Ns, nstcobs=Ws, family=np.array(fam), tag=np.array(tag), u=U, p=Pp, c=Cc, y=Y,
                            f=f, grad_f=gf, F1=F1, F2=F2, psi=psi, grad_psi=gp)
    counts = {k: fam.count(k) for k in sorted(set(fam))}
    groups = sorted({(int(w), int(n)) for w, n in zip(Ws, Ns)})
    print(f"{C} cases {counts}, (nstcobs, N) groups {groups} -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
