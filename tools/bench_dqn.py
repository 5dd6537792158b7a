#!/usr/bin/env python3
"""Benchmark of the fused DQN update (csrc/dqngpu.hip) against the torch update of dqn_train.DqnTrainer.

    python tools/bench_dqn.py [--rounds R] [--buffer ROWS] [--train-timesteps T] [--train-timesteps-full T] [--no-train]

Prints ONE JSON line in the shape of tools/bench_per.py's.  For minibatches of 32 and of 256 rows it times, in updates/s:
the eager update (``DqnTrainer.update``), the graph-replayed update (``update_graphed``, the fastest path before the fused
kernel and the comparison partner), one fused launch per update (``mpcgpu_dqn_step_dev``) and K updates per launch
(``mpcgpu_dqn_train_dev``) at K = 16 and K = 4096.  The first three are timed twice: on a minibatch that is already there, and
with ``ReplayBuffer.sample`` in front as the learner's loop has it -- the K-step launch always draws its rows itself.  The legs
of one size alternate over R rounds; the median is reported with the fastest and slowest round.  Times are host clocks around
work that ends in a device synchronise.  Unless ``--no-train``, three ``tools/train_dqn.py`` runs (4 096 environments) follow:
``--graph --gradient-steps 16``, ``--fused --gradient-steps 16`` (T environment steps each, long enough that start-up does not
carry the figure) and ``--fused --gradient-steps -1`` (one update per transition, fewer environment steps).
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


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def fill(buf, rows, gen, dev):
    for lo in range(0, rows, 65536):
        n = min(65536, rows - lo)
        buf.add(torch.rand(n, 46, device=dev, generator=gen) * 2 - 1, torch.rand(n, 46, device=dev, generator=gen) * 2 - 1,
                torch.randint(0, 9, (n,), device=dev, generator=gen), torch.randn(n, device=dev, generator=gen),
                (torch.rand(n, device=dev, generator=gen) < 0.1).float())


def bench_size(n, buf, gen, rounds, dev):
    torch.manual_seed(0)
    eager = dqn_train.DqnTrainer(device=str(dev), target_update_interval=0)
    graphed = dqn_train.DqnTrainer(device=str(dev), target_update_interval=0)
    graphed.enable_graph(n)
    fused = dqn_fused.FusedDqnTrainer(device=str(dev), target_update_interval=0)
    batch = buf.sample(n, gen)
    # leg -> (one call, updates per call, timed calls, warm-up calls)
    legs = {
        "eager": (lambda: eager.update(batch), 1, 300, 20),
        "graph": (lambda: graphed.update_graphed(batch), 1, 1500, 50),
        "fused_step": (lambda: fused.update(batch), 1, 3000, 50),
        "eager_with_sample": (lambda: eager.update(buf.sample(n, gen)), 1, 300, 20),
        "graph_with_sample": (lambda: graphed.update_graphed(buf.sample(n, gen)), 1, 1500, 50),
        "fused_step_with_sample": (lambda: fused.update(buf.sample(n, gen)), 1, 3000, 50),
        "fused_train_K16": (lambda: fused.train(buf, 16, n), 16, 400, 10),
        "fused_train_K4096": (lambda: fused.train(buf, 4096, n), 4096, 3, 1),
    }
    rates = {k: [] for k in legs}
    for _ in range(rounds):
        for name, (fn, per_call, calls, warmup) in legs.items():
            rates[name].append(per_call / timed(fn, calls, warmup))
    assert bool(torch.isfinite(fused.state).all())
    return {name: {"updates_per_s": statistics.median(r), "us_per_update": 1e6 / statistics.median(r), "min": min(r), "max": max(r)}
            for name, r in rates.items()}


def train_line(extra, timesteps):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_dqn.py"), "--envs", "4096", "--timesteps", str(timesteps)] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env)
    if r.returncode != 0:
        return {"error": r.stderr[-500:], "returncode": r.returncode}
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {"arguments": " ".join(extra), "timesteps": timesteps, "environment_steps_per_s": line["value"], "updates_per_s": line["updates_per_s"],
            "updates": round(line["updates_per_s"] * line["config"]["timesteps_per_gpu"] / line["value"]),
            "updates_per_transition": line["updates_per_s"] / line["value"], "update_path": line["update_path"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buffer", type=int, default=1_000_000, help="rows of the replay buffer the minibatches are drawn from")
    ap.add_argument("--train-timesteps", type=int, default=4_000_000, help="environment steps of the --gradient-steps 16 runs")
    ap.add_argument("--train-timesteps-full", type=int, default=400_000, help="environment steps of the --gradient-steps -1 run")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dqn.py needs the GPU (no fallback)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    buf = dqn_train.ReplayBuffer(args.buffer, 46, dev)
    fill(buf, args.buffer, gen, dev)
    sizes = {f"n{n}": bench_size(n, buf, gen, args.rounds, dev) for n in (32, 256)}
    del buf
    torch.cuda.empty_cache()
    line = {"metric": "fused DQN update: updates/s at batch 256, K = 4096 steps per launch (HIP)",
            "value": sizes["n256"]["fused_train_K4096"]["updates_per_s"], "unit": "updates/s", "n_gpus": 1, "steps": args.rounds,
            "warmup": "per leg", "higher_is_better": True, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"46-16-16-9 Q-network, minibatches of 32 and 256 from {args.buffer} stored rows", "buffer": args.buffer,
                       "rounds": args.rounds},
            "sizes": sizes,
            "ratio_to_graph": {k: {leg: v[leg]["updates_per_s"] / v["graph_with_sample" if "train" in leg or "sample" in leg else "graph"]["updates_per_s"]
                                   for leg in v if leg.startswith("fused")} for k, v in sizes.items()}}
    if not args.no_train:
        line["train_dqn"] = [train_line(extra, steps) for extra, steps in
                             ((["--graph", "--gradient-steps", "16"], args.train_timesteps),
                              (["--fused", "--gradient-steps", "16"], args.train_timesteps),
                              (["--fused", "--gradient-steps", "-1"], args.train_timesteps_full))]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
