#!/usr/bin/env python3
"""Secondary benchmark: the device-resident map stream.

    python tools/bench_maps.py [--variant rays|imgs] [--batch B] [--steps K] [--warmup W] [--cpu-maps N] [--run-steps S]
                               [--refill-every R ...]

``--variant imgs`` runs the same legs on the image environment (BatchedImgsEnv(map_turnover=True): two launches per step).

Prints ONE JSON line per measurement in the shape of tools/bench_plan.py's (metric / value / config / cpu_baseline):

* ``refill``: maps/s of one refill (draw, rings, planner, record: four launches) of B environments with every spare
  missing, next to the host pipeline (path_plan.inflate_spec + rl_env.make_map + rl_env.pack_records) on one core;
* ``refill_vs_step``: the time of those launches next to one fresh-map environment step of B environments;
* ``turnover`` (one line per --refill-every): share of stale resets (a finished row found no spare) and mean episode
  length over --run-steps steps of random actions.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
map_stream = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.map_stream")


def time_launches(fn, steps, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(steps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
    return total / steps


def start_maps(n):
    specs = [map_stream.spec_of(2 ** 40, b) for b in range(16)]
    paths, status = path_plan.plan_reference_paths(specs)
    maps = [rl_env.make_map(path=p, **s) for s, p, st in zip(specs, paths, status) if st == 0][:4]
    return [maps[i % len(maps)] for i in range(n)]


def make_env(B, refill_every, max_episode_steps=400, variant="rays"):
    if variant == "imgs":
        env = rl_env.BatchedImgsEnv(start_maps(B), max_episode_steps=max_episode_steps, capacity=map_stream.DYNAMIC_CAPACITY,
                                    map_turnover=True)
    else:
        env = rl_env.BatchedRaysEnv(start_maps(B), max_episode_steps=max_episode_steps, capacity=map_stream.DYNAMIC_CAPACITY)
    env.enable_fresh_maps(seed=0, refill_every=refill_every)
    env.reset()
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["rays", "imgs"], default="rays")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-maps", type=int, default=40)
    ap.add_argument("--run-steps", type=int, default=2000)
    ap.add_argument("--refill-every", type=int, nargs="*", default=[1, 4, 8, 16, 32])
    args = ap.parse_args()
    B = args.batch
    env = make_env(B, 10 ** 9, variant=args.variant)

    def empty():
        env.spare_ready.zero_()

    refill_s = time_launches(env.refill, args.steps, args.warmup, before=empty)
    status = np.bincount(env.refill_status.cpu().numpy() + 1, minlength=7).tolist()
    line = {"metric": "maps drawn, planned and packed per second (one refill, every spare missing)", "value": B / refill_s,
            "unit": "maps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * refill_s,
            "higher_is_better": True, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{B} generate_map_dynamic maps per refill, one wavefront per map and kernel",
                       "variant": args.variant, "batch_per_gpu": B, "record_bytes": env.records.shape[1] * 8, "status_counts_from_minus_1": status}}
    if args.cpu_maps > 0:
        specs = [map_stream.spec_of(0, b) for b in range(args.cpu_maps)]
        paths, st = path_plan.plan_reference_paths(specs)
        todo = [(s, p) for s, p, ok in zip(specs, paths, st) if ok == 0]
        t0 = time.perf_counter()
        for s, p in todo:
            path_plan.inflate_spec(s)
            rl_env.pack_records([rl_env.make_map(path=p, **s)], limits=map_stream.DYNAMIC_CAPACITY)
        dt = time.perf_counter() - t0
        line["cpu_baseline"] = {"value": len(todo) / dt, "unit": "maps/s", "cores": 1, "kind": "host pipeline",
                                "sample": f"{len(todo)} maps through inflate_spec + make_map + pack_records, {dt:.2f} s (planning not included)"}
    print(json.dumps(line), flush=True)

    acts = torch.randint(0, 9, (B,), device=env.device, dtype=torch.int32)
    step_s = time_launches(lambda: env._launch(acts, env.max_episode_steps), args.steps, args.warmup)
    print(json.dumps({"metric": "one refill of B spares vs one fresh-map environment step of B environments", "variant": args.variant,
                      "batch": B,
                      "refill_ms": 1e3 * refill_s, "env_step_kernel_ms": 1e3 * step_s, "ratio": refill_s / step_s}), flush=True)

    for every in args.refill_every:
        env = make_env(B, every, variant=args.variant)
        gen = torch.Generator(device=env.device)
        gen.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ends = torch.zeros((), dtype=torch.float64, device=env.device)
        for _ in range(args.run_steps):
            a = torch.randint(0, 9, (B,), device=env.device, dtype=torch.int32, generator=gen)
            _, _, term, trunc, _ = env.step(a, auto_reset=True)
            ends += (term | trunc).sum()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loaded, stale = float(env.loaded.sum()), float(env.stale.sum())
        print(json.dumps({"metric": "map turnover under random actions", "variant": args.variant, "batch": B, "refill_every": every,
                          "run_steps": args.run_steps, "episodes": float(ends), "loaded": loaded, "stale": stale,
                          "stale_share": stale / max(loaded + stale, 1.0),
                          "mean_episode_steps": B * args.run_steps / max(float(ends), 1.0),
                          "env_steps_per_s": B * args.run_steps / dt}), flush=True)


if __name__ == "__main__":
    main()
