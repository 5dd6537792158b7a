#!/usr/bin/env python3
"""Secondary benchmark: reference paths planned per second by the visibility-graph kernel.

    python tools/bench_plan.py [--batch B] [--steps K] [--warmup W] [--cpu-seconds S]

Prints ONE JSON line per workload in the shape of tools/bench_env.py's (metric / value / config / cpu_baseline):

* ``fixture``: the 12 maps of tests/golden/planner_maps.npz (the reference's generate_map_mpc), tiled to B;
* ``random_dynamic``: B maps of rl_env.random_dynamic_spec (three inflated boxes in a hall).

A step = one launch that plans B maps, ring records resident in HBM; kernel time by device events.  The CPU leg is the
twin (tests/support/plan_numpy.py, pure Python, one core) -- the only other planner that exists here.  The last line sets
the time to plan B / 100 maps next to one environment step of B environments: roughly the share of environments that end
an episode in a step."""
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
from tests.support import plan_maps, plan_numpy  # noqa: E402


def time_launches(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, e0.elapsed_time(e1) * 1e-3 / steps


def device_batch(planner, maps):
    rec, caps = path_plan.pack_rings([m[0] for m in maps])
    sg = np.array([np.concatenate([m[1], m[2]]) for m in maps])
    return torch.from_numpy(rec).to(planner.device), torch.from_numpy(sg).to(planner.device), caps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    args = ap.parse_args()
    B = args.batch
    planner = path_plan.PathPlanner(0)
    _, fixture_maps, _ = plan_maps.fixture()
    rng = np.random.default_rng(0)
    workloads = {"fixture": [fixture_maps[i % len(fixture_maps)] for i in range(B)],
                 "random_dynamic": [plan_maps.spec_map(rl_env.random_dynamic_spec(rng)) for _ in range(B)]}
    for name, maps in workloads.items():
        rec, sg, caps = device_batch(planner, maps)
        out = planner.plan_dev(rec, sg, **caps)
        status = out[0].cpu().numpy()
        wall, kernel = time_launches(lambda: planner.plan_dev(rec, sg, **caps), args.steps, args.warmup)
        line = {"metric": f"reference paths planned/sec (visibility graph + Dijkstra, {name} maps)", "value": B / wall,
                "unit": "plans/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * wall,
                "higher_is_better": True, "dtype": "f64", "data": "fixture" if name == "fixture" else "synthetic",
                "config": {"workload": f"{B} maps per launch, one workgroup of 256 threads per map", "batch_per_gpu": B,
                           "record_bytes": rec.shape[1] * 8, "ring_vertices_max": caps["n_vert_max"],
                           "status_counts": np.bincount(status, minlength=5).tolist(),
                           "mean_path_nodes": float(out[1].double().mean())},
                "kernel": {"name": "plan_paths_kernel", "kernel_ms": 1e3 * kernel, "plans_per_s_kernel": B / kernel}}
        if args.cpu_seconds > 0:
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < args.cpu_seconds:
                plan_numpy.plan(*maps[n % B])
                n += 1
            dt = time.perf_counter() - t0
            line["cpu_baseline"] = {"value": n / dt, "unit": "plans/s", "cores": 1, "kind": "twin",
                                    "sample": f"{n} maps in tests/support/plan_numpy.py (pure Python), {dt:.1f} s"}
        print(json.dumps(line), flush=True)
    # planning B / 100 maps next to one environment step of B environments
    share = max(1, B // 100)
    rec, sg, caps = device_batch(planner, workloads["random_dynamic"][:share])
    _, plan_s = time_launches(lambda: planner.plan_dev(rec, sg, **caps), args.steps, args.warmup)
    specs = [rl_env.random_dynamic_spec(rng) for _ in range(64)]
    paths, _ = path_plan.plan_reference_paths(specs, planner=planner)
    env_maps = [rl_env.make_map(path=p, **s) for s, p in zip(specs, paths) if p is not None]
    env = rl_env.BatchedRaysEnv([env_maps[i % len(env_maps)] for i in range(B)])
    env.reset()
    acts = torch.randint(0, 9, (B,), device=env.device, dtype=torch.int32)
    _, step_s = time_launches(lambda: env._launch(acts), args.steps, args.warmup)
    print(json.dumps({"metric": "planning B/100 maps vs one environment step of B environments", "batch": B, "maps_planned": share,
                      "plan_kernel_ms": 1e3 * plan_s, "env_step_kernel_ms": 1e3 * step_s, "ratio": plan_s / step_s,
                      "env_steps_per_s": B / step_s}), flush=True)


if __name__ == "__main__":
    main()
