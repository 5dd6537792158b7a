"""cost_grad of a batch of reference vectors in a given table form: the comparison at the tolerance of tests/test_gpu_parity.py,
the spoiler problem that moves a batch to a more general form, and the assertion of the form `last_shape()` reports.  Shared by
tests/test_gpu_cost_edges.py (costgrad_edges.npz) and tests/test_gpu_polygon_golden.py (costgrad_polygons.npz).

A batch b is a dict of unpadded arrays: idx, tag, u, p, c, y and the reference's f, psi, grad_psi, grad_f, F1, F2."""
import numpy as np

from support.edge_cases import KINDS, dyn_rows

RTOL_COST = 1e-11
CHECKED = ("f", "psi", "grad", "F1", "F2", "grad_f", "psi0")


def rel(a, b):
    a, b = np.atleast_2d(np.asarray(a, float)), np.atleast_2d(np.asarray(b, float))
    scale = np.maximum(1.0, np.max(np.abs(b), axis=-1, keepdims=True))
    return np.max(np.abs(a - b) / scale, axis=-1)


def spoiler(cfg, b, kind):
    """one extra problem: a copy of the first case with its last dynamic row replaced by a row 1 km away that is rotated
    ('rot') or changes its shape with the step ('var')"""
    p = b["p"][0].copy()
    rows = dyn_rows(cfg, p)                         # a view into p
    for k in range(cfg.N_hor):
        rows[-1, k] = [1e3, 1e3, 0.5 + (0.01 * k if kind == "var" else 0.0), 0.4, 0.3, 1.0]
    out = dict(b)
    for key, extra in (("u", b["u"][0]), ("p", p), ("c", b["c"][0]), ("y", b["y"][0])):
        out[key] = np.concatenate([b[key], np.asarray(extra)[None] if np.ndim(extra) else np.array([extra])])
    return out


def assert_form(bs, kind):
    s = bs.last_shape()
    assert s["shape_const"] == (kind != "var") and s["axis_aligned"] == (kind == "axis"), (kind, s)


def check(bs, b, what):
    """cost_grad of batch b (its first len(b['idx']) problems are checked) against the reference at RTOL_COST; returns the
    worst relative error of every checked quantity"""
    m = len(b["idx"])
    r = bs.cost_grad(b["u"], b["p"], b["c"], b["y"])
    r0 = bs.cost_grad(b["u"], b["p"])                       # c = 0: psi is f, the gradient is grad f
    errs = dict(f=rel(r["f"][:m, None], b["f"][:, None]), psi=rel(r["psi"][:m, None], b["psi"][:, None]),
                grad=rel(r["grad"][:m], b["grad_psi"]), F1=rel(r["F1"][:m], b["F1"]), F2=rel(r["F2"][:m], b["F2"]),
                grad_f=rel(r0["grad"][:m], b["grad_f"]), psi0=rel(r0["psi"][:m, None], b["f"][:, None]))
    bad = sorted({int(i) for e in errs.values() for i in np.nonzero(~(e < RTOL_COST))[0]})
    assert not bad, f"{what}: " + "; ".join(
        f"{b['tag'][i]}: " + ", ".join(f"{k} {v[i]:.1e}" for k, v in errs.items() if not v[i] < RTOL_COST) for i in bad)
    return {k: float(v.max()) for k, v in errs.items()}


def every_form(bs, cfg, b, kind, what, after=None):
    """the cases of one table kind in their own form, then with a spoiler in each more general one; `after(batch, form)` runs
    behind every check.  Returns {form: worst errors}"""
    worst = {}
    if len(b["idx"]) == 0:
        return worst
    for form in KINDS[KINDS.index(kind):]:
        bb = b if form == kind else spoiler(cfg, b, form)
        worst[form] = check(bs, bb, f"{what} {kind} cases in {form} tables")
        assert_form(bs, form)
        if after is not None:
            after(bb, form)
    return worst
