#!/usr/bin/env python3
"""Benchmark of prioritized replay inside the fused DQN launch (csrc/dqngpu.hip) against the step-by-step path.

    python tools/bench_dqn_per.py [--rounds R] [--buffer ROWS] [--train-timesteps T] [--no-train]

Prints ONE JSON line in the shape of tools/bench_dqn.py's.  On a full prioritized buffer, for minibatches of 32 and of 256 rows
it times, per update:
  leg A  the update round of ``DqnLearner(fused=True, per=True)`` as ``learn`` runs it: ``buffer.sample`` -> ``trainer.update`` ->
         ``buffer.update_priorities``;
  leg B  ``FusedDqnTrainer.train_per`` (``mpcgpu_dqn_train_per_dev``) at K = 16 and K = 4096 steps per launch;
and, for scale, the uniform K-step launch ``train`` at K = 4096 on the same rows.  The legs of one size alternate over R rounds
after every leg's own warm-up; every round is reported, with the median.  Times are host clocks around work that ends in a
device synchronise.  ``accepted`` says whether leg B at K = 4096 is faster than leg A by more than the round-to-round spread
(slowest minus fastest round) of either leg.  Unless ``--no-train``, two ``tools/train_dqn.py`` runs follow (4 096 environments,
batch 256, ``--fused --per --gradient-steps -1``, the same arguments and seed): without and with ``--per-in-kernel``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trajtrack_mpcndqn_rlboost_amd import dqn_fused, dqn_train  # noqa: E402
from tools.bench_dqn import fill, timed  # noqa: E402


def bench_size(n, buf, gen, rounds, dev):
    torch.manual_seed(0)
    stepwise, in_kernel, uniform = (dqn_fused.FusedDqnTrainer(device=str(dev), target_update_interval=0, seed=i) for i in range(3))

    def leg_a():
        batch = buf.sample(n, gen)
        stepwise.update(batch)
        buf.update_priorities(batch["indices"], stepwise.last_td_error)
    # leg -> (one call, updates per call, timed calls, warm-up calls)
    legs = {
        "A_per_stepwise": (leg_a, 1, 3000, 50),
        "B_per_in_kernel_K16": (lambda: in_kernel.train_per(buf, 16, n), 16, 400, 10),
        "B_per_in_kernel_K4096": (lambda: in_kernel.train_per(buf, 4096, n), 4096, 3, 1),
        "uniform_train_K4096": (lambda: uniform.train(buf, 4096, n), 4096, 3, 1),
    }
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for name, (fn, per_call, calls, warmup) in legs.items():
            us[name].append(1e6 * timed(fn, calls, warmup) / per_call)
    for tr in (stepwise, in_kernel, uniform):
        assert bool(torch.isfinite(tr.state).all())
    assert bool(torch.isfinite(buf.sum_tree.tree).all()) and float(buf.sum_tree.tree[0]) > 0.0
    out = {name: {"us_per_update": statistics.median(r), "updates_per_s": 1e6 / statistics.median(r), "rounds_us": r,
                  "spread_us": max(r) - min(r)} for name, r in us.items()}
    a, b = out["A_per_stepwise"], out["B_per_in_kernel_K4096"]
    out["gap_us"] = a["us_per_update"] - b["us_per_update"]
    out["accepted"] = bool(max(b["rounds_us"]) < min(a["rounds_us"]) and out["gap_us"] > max(a["spread_us"], b["spread_us"]))
    print(f"  batch {n}: " + ", ".join(f"{k} {v['us_per_update']:.1f} us" for k, v in out.items() if isinstance(v, dict)), file=sys.stderr, flush=True)
    return out


def train_line(extra, timesteps):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_dqn.py"), "--envs", "4096", "--batch-size", "256", "--timesteps", str(timesteps),
           "--buffer-size", "1000000", "--seed", "0"] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env)
    if r.returncode != 0:
        return {"error": r.stderr[-500:], "returncode": r.returncode}
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(f"  train_dqn.py {' '.join(extra)}: {line['updates_per_s']:.0f} updates/s", file=sys.stderr, flush=True)
    return {"arguments": " ".join(extra), "timesteps": timesteps, "environment_steps_per_s": line["value"], "updates_per_s": line["updates_per_s"],
            "updates": round(line["updates_per_s"] * line["config"]["timesteps_per_gpu"] / line["value"]), "update_path": line["update_path"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buffer", type=int, default=1_000_000, help="capacity of the prioritized replay buffer; it is filled")
    ap.add_argument("--train-timesteps", type=int, default=200_000, help="environment steps of each --gradient-steps -1 run")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dqn_per.py needs the GPU (no fallback)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    buf = dqn_train.ReplayBuffer(args.buffer, 46, dev, per_kwargs={})
    fill(buf, args.buffer, gen, dev)
    assert buf.size == args.buffer
    sizes = {f"n{n}": bench_size(n, buf, gen, args.rounds, dev) for n in (32, 256)}
    del buf
    torch.cuda.empty_cache()
    line = {"metric": "fused DQN update with prioritized replay inside the launch: updates/s at batch 256, K = 4096 (HIP)",
            "value": sizes["n256"]["B_per_in_kernel_K4096"]["updates_per_s"], "unit": "updates/s", "n_gpus": 1, "steps": args.rounds,
            "warmup": "per leg", "higher_is_better": True, "dtype": "f32 (tree f64)", "data": "synthetic",
            "config": {"workload": f"46-16-16-9 Q-network, minibatches of 32 and 256 by priority from {args.buffer} stored rows",
                       "buffer": args.buffer, "rounds": args.rounds},
            "sizes": sizes, "accepted": all(v["accepted"] for v in sizes.values())}
    if not args.no_train:
        common = ["--fused", "--per", "--gradient-steps", "-1"]
        line["train_dqn"] = [train_line(common + extra, args.train_timesteps) for extra in ([], ["--per-in-kernel"])]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
