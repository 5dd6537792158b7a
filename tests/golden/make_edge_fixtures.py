#!/usr/bin/env python3
"""Golden vectors of the cost / gradient path at ties, kinks and unusual shapes, FROM THE REFERENCE ITSELF.

Run in the build container only (needs /root/reference, like make_fixtures.py, whose CasADi / opengen stand-ins,
``load_cfg`` and ``evaluate`` it imports):

    python tests/golden/make_edge_fixtures.py

costgrad_edges.npz holds one record per case, padded to the largest horizon: ``N``, ``family`` (A..F), ``tag`` (what
the case is), ``u [C, 2 Nmax]``, ``p [C, np(Nmax)]``, ``c``, ``y`` and the reference's ``f, grad_f, F1, F2, psi,
grad_psi``.  Row i uses the first 2 N[i] entries of u / y / grad / F1 and the first np(N[i]) of p.

Families (the existing fixtures cover one gentle family: a straight path with one corner near the robot, shape-constant
rotated ellipses, random reals):
  A  exact ties of the path-deviation minimum (u = 0, dyadic geometry).  The reference takes mmin, a left fold of
     fmin: on a tie the EARLIEST segment wins, and its nearest point decides the gradient.  Pairs of tangent segments
     at distance 1 whose partner sits in a lower and in a higher item lane of the step (N = 20, 40, 12, 33, and N = 20
     again for the two-problems-per-wavefront lane split), the steps of N = 40 with a single item lane as a control,
     and V-shaped ties at a shared vertex (equal gradients).
  B  hairpins, retraced and self-crossing paths that start 2-20 m from the robot, zero-length segments mid-path.
  C  dynamic ellipses whose shape changes with the step, axis-aligned constant rows, and both kinds in one problem.
  D  horizons 2, 12, 33, 64.
  E  boundaries: positions exactly on an ellipse, a polygon edge, a fleet circle; F1 + y/max(c,1) on a bound of C;
     u on the bounds of U; c in {0, 1, 1e6}, |y| up to 1e3.
  F  path and obstacles 200-500 m from the origin.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (registers the stand-ins and imports the reference)

OUT = os.path.join(HERE, "costgrad_edges.npz")
DEFAULT_Q = [0.0, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 100.0, 10.0, 20.0]   # yaml defaults (set_work_mode)
AXES = [np.array(v, float) for v in ((1, 0), (0, 1), (-1, 0), (0, -1))]
_cfgs: dict = {}


def cfg_of(N):
    if N not in _cfgs:
        _cfgs[N] = mf.load_cfg(N)
    return _cfgs[N]


def seg_d2(P, s1, s2):
    """the reference's squared distance to a segment (mpc_generator.py:28-36), in float64"""
    d = s2 - s1
    th = np.dot(P - s1, d) / (d[0] ** 2 + d[1] ** 2 + 1e-16)
    t = min(max(th, 0.0), 1.0)
    w = s1 + t * d - P
    return w[0] ** 2 + w[1] ** 2


def path_d2(P, V, k):
    """squared distances of step k's segments k .. N-1 (the last one is zero-length: path_ref[-1] repeated)"""
    N = len(V)
    return np.array([seg_d2(P, V[i], V[min(i + 1, N - 1)]) for i in range(k, N)])


def base_p(cfg, x0, y0, th0, v_init=0.0, w_init=0.0):
    r0, c0, os0, od0, qs0, qd0, npar = mf.offsets(cfg)
    p = np.zeros(npar)
    p[0:3] = [x0, y0, th0]
    p[6:8] = [v_init, w_init]
    p[8:18] = DEFAULT_Q
    p[r0 + 3 * cfg.N_hor:r0 + 4 * cfg.N_hor] = 1.0
    p[qs0:qd0 + cfg.N_hor] = 1e3
    return p


def set_path(cfg, p, V, heading=None):
    r0 = mf.offsets(cfg)[0]
    N = cfg.N_hor
    for k in range(N):
        h = heading[k] if heading is not None else 0.0
        p[r0 + 3 * k:r0 + 3 * k + 3] = [V[k][0], V[k][1], h]
    p[3:5] = V[-1]


def set_dyn(cfg, p, i, rows):
    """rows: N x (cx, cy, rx, ry, ang, alpha)"""
    od0 = mf.offsets(cfg)[3]
    N = cfg.N_hor
    for k in range(N):
        p[od0 + i * 6 * N + 6 * k:od0 + i * 6 * N + 6 * k + 6] = rows[k]


def set_fleet(cfg, p, j, xy):
    c0 = mf.offsets(cfg)[1]
    N = cfg.N_hor
    for k in range(N):
        p[c0 + j * 3 * N + 3 * k:c0 + j * 3 * N + 3 * k + 3] = [xy[k][0], xy[k][1], 0.0]


def set_box(cfg, p, o, x0, x1, y0, y1):
    os0 = mf.offsets(cfg)[2]
    b, a0, a1 = mf.rect_halfspaces(x0, x1, y0, y1)
    p[os0 + 12 * o:os0 + 12 * o + 12] = b + a0 + a1


# --------------------------------------------------------------------------------------------
# family A: exact ties of the path minimum
# --------------------------------------------------------------------------------------------
def tie_vertices(N, P, specials, rng):
    """Vertices r_0 .. r_{N-1} with the given segments fixed (index -> (s1, s2)); every other vertex is pushed away
    from P: radially out of a fixed neighbour, else into a far cluster."""
    V = [None] * N
    for i, (s1, s2) in specials.items():
        for j, q in ((i, s1), (i + 1, s2)):
            assert V[j] is None or np.array_equal(V[j], q), (i, j)
            V[j] = np.array(q, float)
    ang = rng.integers(0, 8) * np.pi / 4
    C = P + np.round(np.array([np.cos(ang), np.sin(ang)]) * 14.0 * 4) / 4
    fixed = [v is not None for v in V]
    for j in range(N):
        if fixed[j]:
            continue
        if j > 0 and fixed[j - 1]:
            V[j] = P + 4.0 * (V[j - 1] - P)
        elif j + 1 < N and fixed[j + 1]:
            V[j] = P + 4.0 * (V[j + 1] - P)
        else:
            V[j] = C + rng.integers(-4, 5, 2) / 4.0
    return V


def tangent(P, n, t, h):
    """segment tangent to the unit circle around P at P + n, direction t, half-length h"""
    T = P + n
    return (T - h * t, T + h * t)


def tie_case(N, k0, i1, i2, kind, rng):
    """u = 0: every predicted position is p[0:2] = P.  At step k0 the minimum over segments >= k0 is d^2 = 1, attained
    EXACTLY by segments i1 < i2 and by no other; kind 'distinct': different nearest points (opposite or orthogonal
    gradients), 'vertex': a V at a shared vertex (i2 = i1 + 1, same nearest point, equal gradients)."""
    cfg = cfg_of(N)
    for _ in range(200):
        P = rng.integers(-12, 13, 2) / 4.0
        if np.hypot(*P) < 1.5:
            continue
        specials = {}
        if kind == "vertex":
            assert i2 == i1 + 1
            n = AXES[rng.integers(4)]
            t = np.array([-n[1], n[0]]) * rng.choice([-1.0, 1.0])
            V0 = P + n
            specials[i1] = (V0 + n + t, V0)
            specials[i2] = (V0, V0 + n - t)
        else:
            a, b = rng.choice(4, 2, replace=False)
            n1, n2 = AXES[a], AXES[b]
            if i2 == i1 + 1:          # a corner: seg i1 ends where seg i2 starts (needs orthogonal normals)
                if abs(np.dot(n1, n2)) > 0:
                    continue
                specials[i1] = tangent(P, n1, n2, 1.0)
                specials[i2] = tangent(P, n2, -n1, 1.0)
            else:
                for i, n in ((i1, n1), (i2, n2)):
                    t = np.array([-n[1], n[0]]) * rng.choice([-1.0, 1.0])
                    specials[i] = tangent(P, n, t, float(rng.choice([1.0, 2.0])))
        try:
            V = tie_vertices(N, P, specials, rng)
        except AssertionError:
            continue
        d = path_d2(P, V, k0)
        others = np.delete(d, [i1 - k0, i2 - k0])
        if not (d[i1 - k0] == 1.0 and d[i2 - k0] == 1.0 and others.min() > 1.25):
            continue
        break
    else:
        raise RuntimeError(f"no tie geometry for N={N} k0={k0} ({i1}, {i2})")
    th0 = float(rng.choice([np.pi / 2, -np.pi / 2, 0.0, rng.uniform(-np.pi, np.pi)]))
    p = base_p(cfg, P[0], P[1], th0, v_init=float(rng.choice([0.0, 0.25])))
    set_path(cfg, p, V)
    c = float(rng.choice([0.0, 10.0]))
    y = np.zeros(2 * N)
    return np.zeros(2 * N), p, c, y


def lane_of(N, k, i, pw=64):
    """item lane (sub index) that holds segment i of step k in eval_point's split (pw = lanes of one problem)"""
    uniform = (pw % N) * 5 <= N and N in (20, 40) and pw == 64
    lps = pw // N if uniform else (pw - 1 - k) // N + 1
    return (i - k) % lps


def family_A(rng):
    cases = []
    spec = [
        # (N, k0, i1, i2, kind, what)
        (20, 0, 1, 3, "distinct", "N20 partner in a lower lane"),
        (20, 0, 2, 4, "distinct", "N20 partner in a lower lane"),
        (20, 5, 6, 8, "distinct", "N20 partner in a lower lane"),
        (20, 7, 9, 13, "distinct", "N20 partner in a lower lane"),
        (20, 0, 0, 1, "distinct", "N20 corner, partner in a higher lane"),
        (20, 10, 10, 11, "distinct", "N20 corner, partner in a higher lane"),
        (20, 3, 3, 6, "distinct", "N20 same lane"),
        (20, 12, 13, 18, "distinct", "N20 late steps"),
        (20, 4, 8, 9, "vertex", "N20 shared vertex"),
        (20, 0, 16, 17, "vertex", "N20 shared vertex"),
        (40, 0, 1, 2, "distinct", "N40 two-lane steps, partner in a lower lane"),
        (40, 10, 11, 14, "distinct", "N40 two-lane steps, partner in a lower lane"),
        (40, 20, 22, 23, "distinct", "N40 two-lane steps, corner"),
        (40, 5, 5, 8, "distinct", "N40 two-lane steps, partner in a higher lane"),
        (40, 2, 6, 7, "vertex", "N40 shared vertex"),
        # control: both segments in steps 24-39 (one item lane each), an even index gap (one lane at steps 0-23 too)
        (40, 24, 25, 27, "distinct", "N40 one-lane steps (control)"),
        (40, 24, 31, 35, "distinct", "N40 one-lane steps (control)"),
        (40, 26, 28, 29, "vertex", "N40 one-lane steps (control), shared vertex"),
        (12, 0, 1, 6, "distinct", "N12 runtime horizon, partner in a lower lane"),
        (12, 4, 5, 9, "distinct", "N12 runtime horizon, partner in a lower lane"),
        (12, 0, 2, 3, "distinct", "N12 runtime horizon, corner"),
        (12, 1, 4, 5, "vertex", "N12 shared vertex"),
        (33, 0, 1, 2, "distinct", "N33 runtime horizon, partner in a lower lane"),
        (33, 29, 30, 31, "distinct", "N33 runtime horizon, late corner"),
        (33, 3, 5, 8, "distinct", "N33 runtime horizon, partner in a lower lane"),
        (20, 0, 1, 2, "distinct", "N20 duo split (2 lanes/step), partner in a lower lane"),
        (20, 6, 7, 10, "distinct", "N20 duo split, partner in a lower lane"),
        (20, 12, 13, 15, "distinct", "N20 duo split one-lane steps"),
    ]
    for N, k0, i1, i2, kind, what in spec:
        u, p, c, y = tie_case(N, k0, i1, i2, kind, rng)
        lanes = f"lanes@k0 {lane_of(N, k0, i1)}/{lane_of(N, k0, i2)}"
        if N == 20:     # and in the two-problems-per-wavefront layout (32 lanes per problem)
            lanes += f", pairing=2: {lane_of(N, k0, i1, 32)}/{lane_of(N, k0, i2, 32)}"
        cases.append((N, "A", f"{what}: k0={k0} segs {i1},{i2} {lanes}", u, p, c, y))
    return cases


# --------------------------------------------------------------------------------------------
# generic scene pieces (families B-F)
# --------------------------------------------------------------------------------------------
def rand_u(rng, N, scale=1.0):
    v = rng.uniform(-0.5, 1.5, N) * scale
    w = rng.uniform(-0.5, 0.5, N) * scale
    return np.stack([v, w], axis=1).reshape(-1)


def add_obstacles(cfg, p, rng, centre, spread, n_dyn=3, n_stc=2, n_other=2, kinds=("rot",)):
    N = cfg.N_hor
    for j in range(n_other):
        b = centre + rng.uniform(-spread, spread, 2)
        vel = rng.uniform(-0.05, 0.05, 2)
        set_fleet(cfg, p, j, [b + vel * k for k in range(N)])
    for o in range(n_stc):
        cx, cy = centre + rng.uniform(-spread, spread, 2)
        hx, hy = rng.uniform(0.3, 1.0, 2)
        set_box(cfg, p, o, cx - hx, cx + hx, cy - hy, cy + hy)
    for i in range(n_dyn):
        kind = kinds[i % len(kinds)]
        b = centre + rng.uniform(-spread, spread, 2)
        vel = rng.uniform(-0.15, 0.15, 2)
        rx, ry = rng.uniform(0.3, 1.6, 2)
        ang = 0.0 if kind == "axis" else rng.uniform(-np.pi, np.pi)
        alpha = rng.uniform(0.2, 1.0)       # constant over the horizon: the library's shape-constant test includes alpha
        rows = []
        for k in range(N):
            if kind == "var":     # shape changes with the step
                rows.append([b[0] + vel[0] * k, b[1] + vel[1] * k, rx * (1 + 0.05 * k), ry * (1 - 0.01 * k),
                             ang + 0.1 * k, rng.uniform(0.2, 1.0)])
            else:
                rows.append([b[0] + vel[0] * k, b[1] + vel[1] * k, rx, ry, ang, alpha])
        set_dyn(cfg, p, i, rows)


def curve(rng, start, head, N, step=(0.24, 1.0), hairpin_at=None, loop=False):
    pts, hs = [], []
    x = np.array(start, float)
    for k in range(N):
        if hairpin_at is not None and k == hairpin_at:
            head += np.pi
        elif loop:
            head += 2 * np.pi / max(N // 2, 2) + rng.uniform(-0.1, 0.1)
        else:
            head += rng.uniform(-0.3, 0.3)
        x = x + rng.uniform(*step) * np.array([np.cos(head), np.sin(head)])
        pts.append(x.copy()); hs.append(head)
    return pts, hs


def family_B(rng):
    cases = []
    for N in (20, 40, 20, 40, 33):
        cfg = cfg_of(N)
        for form in ("hairpin", "loop", "retrace"):
            P = rng.uniform(-3, 3, 2)
            R = rng.uniform(2.0, 20.0)
            a = rng.uniform(-np.pi, np.pi)
            start = P + R * np.array([np.cos(a), np.sin(a)])
            head = a + np.pi + rng.uniform(-0.3, 0.3)          # towards the robot
            zero_u = form == "retrace"
            if form == "retrace":      # out and back on the same dyadic line, robot at P exactly: equal-distance twins
                P = rng.integers(-8, 9, 2) / 4.0
                d = AXES[rng.integers(4)]
                off = np.array([-d[1], d[0]])
                half = (N + 1) // 2
                pts = [P + off + (R // 1 - j) * d * 0.5 for j in range(half)]
                pts += pts[::-1][:N - half]
                hs = [0.0] * N
            else:
                pts, hs = curve(rng, start, head, N, step=(0.24, max(0.3, R / N * 1.5)),
                                hairpin_at=N // 2 if form == "hairpin" else None, loop=form == "loop")
            # zero-length segments in the middle of the path
            for j in rng.choice(np.arange(2, N - 2), 2, replace=False):
                pts[j + 1] = pts[j].copy()
            p = base_p(cfg, P[0], P[1], rng.uniform(-np.pi, np.pi), rng.uniform(0, 1.0), rng.uniform(-0.3, 0.3))
            set_path(cfg, p, pts, hs)
            add_obstacles(cfg, p, rng, np.mean(pts, axis=0), 2.0, n_dyn=int(rng.integers(0, 4)))
            u = np.zeros(2 * N) if zero_u else rand_u(rng, N)
            c = float(rng.choice([0.0, 10.0, 250.0]))
            y = rng.uniform(-3, 3, 2 * N) * (rng.random() < 0.5)
            cases.append((N, "B", f"{form} N{N} R={R:.1f}", u, p, c, y))
    return cases


def near_path_case(N, rng, kinds, tag, origin=(0.0, 0.0), fam="C"):
    cfg = cfg_of(N)
    o = np.array(origin, float)
    P = o + rng.uniform(-2, 2, 2)
    th = rng.uniform(-np.pi, np.pi)
    pts, hs = curve(rng, P, th, N, step=(0.2, 0.3))
    p = base_p(cfg, P[0], P[1], th, rng.uniform(0, 1.2), rng.uniform(-0.3, 0.3))
    set_path(cfg, p, pts, hs)
    add_obstacles(cfg, p, rng, pts[N // 3], 1.0, n_dyn=len(kinds), n_stc=int(rng.integers(0, 4)),
                  n_other=int(rng.integers(0, 3)), kinds=kinds)
    u = rand_u(rng, N)
    c = float(rng.choice([1.0, 10.0, 1250.0]))
    y = rng.uniform(-5, 5, 2 * N)
    return (N, fam, tag, u, p, c, y)


def family_C(rng):
    cases = []
    for N in (20, 40, 12):
        for _ in range(2):
            cases.append(near_path_case(N, rng, ("var", "var", "rot"), f"general tables N{N}"))
            cases.append(near_path_case(N, rng, ("axis", "axis", "axis"), f"axis-aligned tables N{N}"))
            cases.append(near_path_case(N, rng, ("axis", "var", "rot", "axis"), f"mixed rows N{N}"))
    return cases


def family_D(rng):
    cases = []
    for N in (2, 12, 33, 64):
        for kinds in (("rot", "rot"), ("axis",), ("var", "axis", "rot")):
            cases.append(near_path_case(N, rng, kinds, f"horizon N{N} {'/'.join(kinds)}", fam="D"))
    return cases


def on_boundary(x, r, margin, side):
    """(rx, cx) with x - cx == side * ((rx + margin) + 1e-6) exactly in float64 (the reference's ellipse denominators,
    mpc_generator.py:42,271): P lies exactly on the boundary of the axis-aligned ellipse, on side `side` of its centre"""
    rx = r
    for _ in range(256):
        a = (rx + margin) + 1e-6
        cx = x - side * a
        if side * (x - cx) == a:
            return float(rx), float(cx)
        rx = np.nextafter(rx, np.inf)
    raise RuntimeError("no exact boundary")


def family_E(rng):
    cases = []
    for N in (20, 40):
        cfg = cfg_of(N)
        P = np.array([1.0, -1.75])
        # (1) on a fleet circle (|d| = vehicle_width = 0.5: the hinge 1000 * fmax(0, W^2 - d^2) at its kink), on a polygon
        #     edge, on an axis-aligned ellipse boundary (x - cx == fl(rx + 1e-6))
        p = base_p(cfg, P[0], P[1], 0.75, 0.2, 0.0)            # v_init = 0.2: F1 = (0 - 0.2) / 0.2 = -1 = lin_acc_min
        set_path(cfg, p, [P + np.array([0.25 * (k + 1), 0.5]) for k in range(N)])
        set_fleet(cfg, p, 0, [P + np.array([0.5, 0.0])] * N)
        set_fleet(cfg, p, 1, [P + np.array([0.0, -0.5])] * N)
        set_box(cfg, p, 0, P[0] - 1.0, P[0] + 0.0, P[1] - 0.5, P[1] + 0.5)     # P on the right edge
        set_box(cfg, p, 1, P[0] - 0.25, P[0] + 0.25, P[1], P[1] + 1.0)        # P on the bottom edge
        rx, cx = on_boundary(P[0], 0.625, 0.0, 1.0)             # hard ellipse: P on its boundary
        set_dyn(cfg, p, 0, [[cx, P[1], rx, 0.5, 0.0, 1.0]] * N)
        rs, cs = on_boundary(P[0], 0.55, 0.2, 1.0)              # cost ellipse (rx + social margin) on P as well
        set_dyn(cfg, p, 1, [[cs, P[1], rs, 0.5, 0.0, 1.0]] * N)
        for c, ys in ((0.0, 0.0), (1.0, 0.0), (1e6, 0.0), (10.0, 1e3)):
            y = np.zeros(2 * N)
            if ys:
                y[:] = np.linspace(-ys, ys, 2 * N)
            cases.append((N, "E", f"on fleet circle / polygon edge / ellipse boundary, c={c:g} |y|<={ys:g}",
                          np.zeros(2 * N), p.copy(), c, y))
        # (2) F1 + y / max(c, 1) exactly on a bound of C: u on the bounds of U, v_init / w_init chosen so that
        #     acc = (v_k - v_{k-1}) / ts sits on [-1, 1] and the angular one on [-3, 3] after the multiplier shift
        p2 = base_p(cfg, P[0], P[1], 0.25, 1.3, 0.0)
        set_path(cfg, p2, [P + np.array([0.25 * (k + 1), 0.0]) for k in range(N)])
        v = np.where(np.arange(N) % 2 == 0, 1.5, -0.5)          # on the bounds of U; accelerations -10, +10 ...
        w = np.where(np.arange(N) % 3 == 0, 0.5, -0.5)
        u = np.stack([v, w], axis=1).reshape(-1)
        for c in (1.0, 4.0, 1e6):
            F1 = np.concatenate([(v - np.concatenate([[1.3], v[:-1]])) / 0.2, (w - np.concatenate([[0.0], w[:-1]])) / 0.2])
            lo = np.array([-1.0] * N + [-3.0] * N)
            hi = np.array([1.0] * N + [3.0] * N)
            target = np.where(np.arange(2 * N) % 2 == 0, lo, hi)
            y = (target - F1) * max(c, 1.0)                      # F1 + y/max(c,1) == bound (up to the rounding of the
            cases.append((N, "E", f"F1 + y/max(c,1) on the bounds of C, u on the bounds of U, c={c:g}",  # reference)
                          u.copy(), p2.copy(), c, y))
    return cases


def family_F(rng):
    cases = []
    for N in (20, 40, 33):
        for _ in range(3):
            r = rng.uniform(200.0, 500.0)
            a = rng.uniform(-np.pi, np.pi)
            kinds = [("rot", "rot"), ("axis", "axis"), ("var", "rot")][len(cases) % 3]
            cases.append(near_path_case(N, rng, kinds, f"large coordinates N{N} |x|~{r:.0f} m",
                                        origin=(r * np.cos(a), r * np.sin(a)), fam="F"))
    return cases


# --------------------------------------------------------------------------------------------
def savez_deterministic(path, **arrays):
    """np.savez_compressed without the wall-clock time stamps in the zip headers: reruns give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    rng = np.random.default_rng(20261015)
    cases = family_A(rng) + family_B(rng) + family_C(rng) + family_D(rng) + family_E(rng) + family_F(rng)
    Nmax = max(cs[0] for cs in cases)
    npmax = mf.np_of(cfg_of(Nmax))
    C = len(cases)
    n2 = cfg_of(20).Ndynobs
    U = np.zeros((C, 2 * Nmax)); Pp = np.zeros((C, npmax)); Y = np.zeros((C, 2 * Nmax)); Cc = np.zeros(C)
    f = np.zeros(C); psi = np.zeros(C); gf = np.zeros((C, 2 * Nmax)); gp = np.zeros((C, 2 * Nmax))
    F1 = np.zeros((C, 2 * Nmax)); F2 = np.zeros((C, n2))
    Ns = np.zeros(C, np.int32)
    fam, tag = [], []
    for i, (N, fm, tg, u, p, c, y) in enumerate(cases):
        cfg = cfg_of(N)
        assert p.size == mf.np_of(cfg) and u.size == y.size == 2 * N
        r = mf.evaluate(cfg, u, p, c, y)
        assert np.all(np.isfinite(r["grad_psi"])) and np.isfinite(r["psi"]), tg
        Ns[i] = N; U[i, :2 * N] = u; Pp[i, :p.size] = p; Y[i, :2 * N] = y; Cc[i] = c
        f[i] = r["f"]; psi[i] = r["psi"]
        gf[i, :2 * N] = r["grad_f"]; gp[i, :2 * N] = r["grad_psi"]
        F1[i, :2 * N] = r["F1"]; F2[i] = r["F2"]
        fam.append(fm); tag.append(tg)
    savez_deterministic(OUT, N=Ns, family=np.array(fam), tag=np.array(tag), u=U, p=Pp, c=Cc, y=Y,
                        f=f, grad_f=gf, F1=F1, F2=F2, psi=psi, grad_psi=gp)
    counts = {k: fam.count(k) for k in sorted(set(fam))}
    print(f"{C} cases {counts} -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
