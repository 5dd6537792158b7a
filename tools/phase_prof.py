#!/usr/bin/env python3
"""Phase-cycle breakdown of the throughput solver kernel (needs a -DMPC_PROFILE build: MPCGPU_LIB=<that .so>).

Runs with MPCGPU_OPT_TAIL_PROMOTION OFF and the latency kernel off: since round 6 the latency kernel writes its own marks into the
slots read here as the throughput kernel's evaluation counts, and a launch that promotes its tail mixes the two (VERDICT.md, weak
point 11; profiles/r06_phase_table.txt is polluted that way).  The evaluations per solve summed from the profile must equal the
solver's own count of the same call (last_eval_counts: the mean_psi_evaluations of bench.py) within 1 %."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trajtrack_mpcndqn_rlboost_amd import MpcConfig, BatchSolver, scenes
B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
NH = int(sys.argv[2]) if len(sys.argv) > 2 else 20
cfg = MpcConfig(N_hor=NH)
bs = BatchSolver(cfg, latency_batch=0, tail_promotion=0)
sc = scenes.make_batch(cfg, B, n_dyn=8, seed=1236)
print(f"N_hor {NH}  B {B}  8 dynamic obstacles (benchmark scene family)")
res = bs.solve(sc["p"])
out = (C.c_double * 24)()
bs._L.mpcgpu_debug_read_prof.argtypes = [C.POINTER(C.c_double)]
bs._L.mpcgpu_debug_read_prof(out)
res = bs.solve(sc["p"])
bs._L.mpcgpu_debug_read_prof(out)
t = np.array(out[:])
names = ["headings", "positions+publish", "segments", "fleet+static", "dynamic", "pads+constraint sums", "phase B",
         "combine", "vector terms+psi", "adjoint"]
states = ["INIT0", "INIT1", "LIP", "NOLS", "LS", "OUTER"]
evals = t[16:22].sum()
tot = t[:16].sum() + t[22]
mean_psi = float(bs.last_eval_counts(B)[0].mean())
assert bs.last_tail_promotion()[1] == 0, "problems were promoted to the latency kernel: its marks pollute the table"
assert abs(evals / B - mean_psi) <= 0.01 * mean_psi, f"profile counts {evals / B:.1f} evaluations per solve, the solver {mean_psi:.1f}"
print(f"solve_ms {bs.last_timing()['solve_ms']:.1f}  evals/solve {evals / B:.0f}  cycles/solve {tot / B:.3g}  cycles/eval(all incl.) {tot / evals:.0f}")
for i, n in enumerate(names):
    print(f"  eval: {n:22s} {t[i] / evals:8.0f} cyc/eval  {100 * t[i] / tot:5.1f} %")
for i, n in enumerate(states):
    c = t[16 + i]
    print(f"  logic before {n:6s} evals {c / B:8.0f}/solve  {t[10 + i] / max(c, 1):8.0f} cyc each  {100 * t[10 + i] / tot:5.1f} %")
print(f"  reference segments beyond the two nearest: the suffix-circle loop was entered (by at least one lane) in {t[23] / evals:.3f} of the evaluations")
