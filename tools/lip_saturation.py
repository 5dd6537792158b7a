#!/usr/bin/env python3
"""How many Lipschitz-test evaluations of psi(u_half) cannot matter (MPC_LIP_SKIP, csrc/mpc_kernels.hpp), from the oracle's decision
trace on the CPU.  A PANOC step evaluates psi(u_half) once, and once more after every update L <- 2L; the test that reads the number is
`psi(u_half) > bound && updates < 10 && L < 1e9`.  An evaluation is DEAD when the last two conditions are false before it runs:

  * the first evaluation of a step whose L before the step is >= 1e9;
  * the re-evaluation after an update that left L >= 1e9, or after the tenth update.

The trace (oracle.solve_trace) has one record per step with L AFTER the step (field 3) and the number of updates (field 7); L only
doubles inside a step, so L before the step is L / 2^updates, exactly.  Prints the share per problem and the totals.

usage: lip_saturation.py [--family benchmark] [--N 20] [--problems 256] [--n-dyn 8] [--seed 1234] [--max-inner K] [--penalty-stall either|both]
                         [--init-penalty C]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_LIP = 1e9       # K_MAX_LIP of the kernels, MAX_LIPSCHITZ of the oracle
MAX_LIP_IT = 10


def dead_in_trace(trace):
    """(steps, Lipschitz-test evaluations, dead ones) of one solve's trace [steps, 12]"""
    L_after, n_up = trace[:, 3], trace[:, 7].astype(int)
    evals = dead = 0
    for La, k in zip(L_after, n_up):
        L = La / 2.0 ** k
        for j in range(k + 1):          # evaluation j runs after j updates
            evals += 1
            dead += int(L >= MAX_LIP or j >= MAX_LIP_IT)
            L *= 2.0
    return len(trace), evals, dead


def dead_evaluations(cfg, p, u0=None):
    """Per problem of the batch p [B, np] under MpcConfig cfg: arrays (steps, evals, dead) from oracle.solve_trace."""
    import oracle
    ocfg = oracle.OracleConfig.from_dict(cfg.solver_dict())
    cap = (int(cfg.solver_max_inner_iterations) + 2) * int(cfg.solver_max_outer_iterations)   # (the cap counts completed iterations: one step more)
    out = []
    for b in range(p.shape[0]):
        _, _, tr, steps = oracle.solve_trace(ocfg, p[b], None if u0 is None else u0[b], cap=cap)
        assert steps <= cap, (steps, cap)
        out.append(dead_in_trace(tr))
    return tuple(np.array(c) for c in zip(*out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="benchmark")
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--n-dyn", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max-inner", type=int, default=None, help="solver_max_inner_iterations (default: the configuration's)")
    ap.add_argument("--penalty-stall", choices=("either", "both"), default=None)
    ap.add_argument("--init-penalty", type=float, default=None, help="solver_initial_penalty (default: the configuration's)")
    ap.add_argument("--quiet", action="store_true", help="totals only")
    a = ap.parse_args()
    from trajtrack_mpcndqn_rlboost_amd import MpcConfig, scenes
    kw = {}
    if a.max_inner is not None:
        kw["solver_max_inner_iterations"] = a.max_inner
    if a.penalty_stall is not None:
        kw["solver_penalty_stall"] = a.penalty_stall
    if a.init_penalty is not None:
        kw["solver_initial_penalty"] = a.init_penalty
    cfg = MpcConfig(N_hor=a.N, **kw)
    p = scenes.make_family(cfg, a.problems, a.family, n_dyn=a.n_dyn, seed=a.seed)["p"]
    steps, evals, dead = dead_evaluations(cfg, p)
    if not a.quiet:
        print("problem   steps  lip evals    dead   share")
        for b in range(a.problems):
            print(f"{b:7d} {steps[b]:7d} {evals[b]:10d} {dead[b]:7d} {100.0 * dead[b] / max(evals[b], 1):6.1f} %")
    share = dead / np.maximum(evals, 1)
    print(f"family {a.family}, N_hor {a.N}, {a.problems} problems, n_dyn {a.n_dyn}, seed {a.seed}, {kw or 'default settings'}")
    print(f"steps {steps.sum()}  Lipschitz-test evaluations {evals.sum()}  dead {dead.sum()} = {100.0 * dead.sum() / max(evals.sum(), 1):.1f} %  "
          f"problems affected {int((dead > 0).sum())} of {a.problems} ({int((share > 0.10).sum())} above 10 %; per-problem share up to "
          f"{100.0 * share.max():.0f} %)")


if __name__ == "__main__":
    main()
