#!/usr/bin/env python3
"""Benchmark of the prioritized-replay sum tree (csrc/pergpu.hip) against the same semantics in torch operations.

    python tools/bench_per.py [--capacity C] [--n N] [--add-rows R] [--cycles K] [--warmup W]

Prints ONE JSON line in the shape of tools/bench_env.py's.  A cycle = one ``sample`` of N rows + one ``update`` of those rows
with random TD errors on a full tree of C leaves; after the cycles, ``add`` of R rows is timed on its own.  The baseline leg
is what torch offers without a tree, on the same device: cumulative sum over the C leaves + ``searchsorted`` of the N
stratified draws + the weights, ``index_put`` of the new priorities (last row wins is NOT guaranteed there), and for add a
max over the leaves + a slice assignment.  Times are host clocks around work that ends in a device synchronise.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trajtrack_mpcndqn_rlboost_amd.per_tree import SumTree  # noqa: E402


def timed(fn, cycles, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(cycles):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--add-rows", type=int, default=4096)
    ap.add_argument("--cycles", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_per.py needs the GPU (no fallback)")
    dev, C, n = torch.device("cuda", 0), args.capacity, args.n
    gen = torch.Generator(device=dev).manual_seed(0)
    tree = SumTree(C, dev)
    for pos in range(0, C, 32768):                   # a full buffer with spread priorities
        tree.add(pos, min(32768, C - pos), pos)
    for lo in range(0, C, 4096):
        idx = torch.arange(lo, min(lo + 4096, C), device=dev) + C - 1
        tree.update(idx, torch.randn(idx.numel(), device=dev, generator=gen))
    u = torch.rand(args.cycles + args.warmup, n, dtype=torch.float64, device=dev, generator=gen)
    td = torch.randn(args.cycles + args.warmup, n, device=dev, generator=gen)
    step = [0]

    def hip_cycle():
        k = step[0] = (step[0] + 1) % u.shape[0]
        idx, ring, w = tree.sample(u[k], C)
        tree.update(idx, td[k])

    pos = [0]

    def hip_add():
        tree.add(pos[0], args.add_rows, C)
        pos[0] = (pos[0] + args.add_rows) % C

    leaves = tree.tree[C - 1:].clone()
    alpha, beta, eps = 0.3, 0.4, 1e-3
    strata = torch.arange(n, dtype=torch.float64, device=dev)
    max_p = torch.ones((), dtype=torch.float64, device=dev)

    def torch_cycle():
        k = step[0] = (step[0] + 1) % u.shape[0]
        cum = torch.cumsum(leaves, 0)
        total = cum[-1]
        s = (strata + u[k]) * (total / n)
        ring = torch.searchsorted(cum, s).clamp_(max=C - 1)
        w = (C * leaves[ring] / total) ** (-beta)
        w = (w / w.max()).float()
        leaves.index_put_((ring,), (td[k].double().abs() + eps) ** alpha)

    def torch_add():
        max_p.copy_(leaves.max())
        rows = (pos[0] + torch.arange(args.add_rows, device=dev)) % C
        leaves[rows] = max_p
        pos[0] = (pos[0] + args.add_rows) % C

    t_hip, t_torch = timed(hip_cycle, args.cycles, args.warmup), timed(torch_cycle, args.cycles, args.warmup)
    a_hip, a_torch = timed(hip_add, max(args.cycles // 4, 1), args.warmup), timed(torch_add, max(args.cycles // 4, 1), args.warmup)
    line = {"metric": "prioritized replay: sample + update cycles/s (HIP sum tree)", "value": 1.0 / t_hip, "unit": "cycles/s",
            "n_gpus": 1, "steps": args.cycles, "warmup": args.warmup, "us_per_cycle": 1e6 * t_hip, "higher_is_better": True,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"full tree of {C} leaves, sample {n} + update {n} per cycle; add of {args.add_rows} rows",
                       "capacity": C, "n": n, "add_rows": args.add_rows},
            "add": {"value": args.add_rows / a_hip, "unit": "rows/s", "us_per_call": 1e6 * a_hip, "calls_per_s": 1.0 / a_hip},
            "torch_baseline": {"kind": "cumsum + searchsorted + index_put on the same device", "cycles_per_s": 1.0 / t_torch,
                               "us_per_cycle": 1e6 * t_torch, "add_rows_per_s": args.add_rows / a_torch,
                               "add_us_per_call": 1e6 * a_torch},
            "ratio_cycles": t_torch / t_hip, "ratio_add": a_torch / a_hip}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
