"""Table forms of the edge-case vectors (tests/golden/costgrad_edges.npz): which form of the dynamic-obstacle tables a
problem alone would be evaluated in.  Shared by tests/test_oracle_edges.py and tests/test_gpu_cost_edges.py."""
import numpy as np

KINDS = ("axis", "rot", "var")      # axis-aligned < shape-constant rotated < general: a batch takes its least regular problem's


def dyn_rows(cfg, p):
    """[Ndynobs, N, 6] view of the dynamic table of one parameter vector (cx, cy, rx, ry, angle, alpha per row and step)"""
    od = cfg.offsets()["od"]
    return p[od:od + cfg.Ndynobs * cfg.ndynobs * cfg.N_hor].reshape(cfg.Ndynobs, cfg.N_hor, cfg.ndynobs)


def table_kind(cfg, p):
    """the library's rule (table preparation in mpc_kernels.hpp): a row is active when any of its entries is non-zero; the
    tables are general when rx, ry, angle or alpha of a row changes over the horizon, rotated when an active row has a
    non-zero angle, axis-aligned otherwise (no dynamic row at all included)"""
    rows = dyn_rows(cfg, p)
    act = np.any(rows != 0.0, axis=(1, 2))
    if np.any(rows[:, 1:, 2:6] != rows[:, :1, 2:6]):
        return "var"
    return "rot" if np.any(rows[act][:, :, 4] != 0.0) else "axis"
