#!/usr/bin/env python3
"""Greedy evaluation episodes: the host-driven loop of the existing entries against ``evaluate.evaluate_rays``.

    python tools/bench_eval.py [--batches 256,4096] [--episodes 1] [--rounds 3] [--out profiles/eval_bench.txt]

Both legs evaluate the same fixed random parameter vector with eps = 0 on scene 1 of tools/train_dqn.py (``max_episode_steps``
400), from a reset, until every row has ``--episodes`` episodes:

* host: ``collect.act`` -> ``env.step(auto_reset=True)`` -> the episode bookkeeping in torch operations, some forty launches per
  step; the host reads "is every row finished" once per 32 steps and stops at ``episodes * max_episode_steps`` steps;
* kernel: ``evaluate_rays`` with its default ``launch_steps`` (one host read per launch).

They run in ONE process on environments of their own and take turns: host, kernel, host, kernel, ... for ``--rounds`` rounds, each
evaluation timed between two device synchronisations; the two legs' returns, lengths and outcomes are compared bit for bit.
Evaluation steps are the steps the rows made until their last episode ended (the sum of the episode lengths), the same number
for both legs.  A last measurement times ONE launch of the default ``launch_steps`` at the largest batch on an evaluation of four
episodes per row, where rows that run into the time limit make every step of the launch.  Prints one line per batch and ends
with ONE JSON line in the shape of tools/bench_env.py; every round goes to ``--out`` as well."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
collect = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.collect")
evaluate = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.evaluate")
train_dqn = importlib.import_module("tools.train_dqn")
MAX_EPISODE_STEPS = 400
SEED = 7


def host_evaluation(env, theta, E: int):
    """The evaluation as the single-step entries allow it -> (returns, lengths, outcome), each [B, E]."""
    B, dev = env.B, env.device
    returns = torch.zeros(B, E, dtype=torch.float64, device=dev)
    lengths = torch.zeros(B, E, dtype=torch.int32, device=dev)
    outcome = torch.zeros(B, E, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.int64, device=dev)
    ep_return = torch.zeros(B, dtype=torch.float64, device=dev)
    ep_length = torch.zeros(B, dtype=torch.int32, device=dev)
    rows = torch.arange(B, device=dev)
    for r in range(E * MAX_EPISODE_STEPS):
        live = done < E
        if r % 32 == 0 and r and not bool(live.any()):
            break
        actions = collect.act(env, theta, 0.0, SEED, r)
        _, reward, terminated, truncated, _ = env.step(actions, auto_reset=True)
        ended = (terminated | truncated) & live
        ep_return = torch.where(live, ep_return + reward, ep_return)
        ep_length = ep_length + live.to(torch.int32)
        slot = done.clamp(max=E - 1)
        word = ((env.state[:, 26].to(torch.int64) & 7) | (truncated.to(torch.int64) * 8)).to(torch.uint8)
        returns[rows, slot] = torch.where(ended, ep_return, returns[rows, slot])
        lengths[rows, slot] = torch.where(ended, ep_length, lengths[rows, slot])
        outcome[rows, slot] = torch.where(ended, word, outcome[rows, slot])
        ep_return = torch.where(ended, torch.zeros_like(ep_return), ep_return)
        ep_length = torch.where(ended, torch.zeros_like(ep_length), ep_length)
        done = done + ended.to(torch.int64)
    return returns, lengths, outcome


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="a text file that receives every printed line")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    E = args.episodes
    theta = torch.from_numpy(np.random.default_rng(12).uniform(-0.3, 0.3, 1177).astype(np.float32)).to("cuda:0")
    legs = []
    for B in [int(b) for b in args.batches.split(",")]:
        rng = np.random.default_rng(100)
        maps = [train_dqn.scene(rng) for _ in range(B)]
        envs = {"host": rl_env.BatchedRaysEnv(maps, max_episode_steps=MAX_EPISODE_STEPS),
                "kernel": rl_env.BatchedRaysEnv(maps, max_episode_steps=MAX_EPISODE_STEPS)}

        def from_the_start(env):        # reset() keeps the observation memory of the state: cleared, both legs start every round alike
            env.state.zero_()
            env.reset()

        def host():
            from_the_start(envs["host"])
            return host_evaluation(envs["host"], theta, E)

        def kernel():
            from_the_start(envs["kernel"])
            res = evaluate.evaluate_rays(envs["kernel"], theta, E, seed=SEED)
            return res["returns"], res["lengths"], res["outcome"]
        host(), kernel()                                                  # warm-up: the library, the allocator
        seconds, same, steps = {"host": [], "kernel": []}, True, 0
        for _ in range(args.rounds):
            results = {}
            for name, fn in (("host", host), ("kernel", kernel)):
                dt, results[name] = timed(fn)
                seconds[name].append(dt)
            same = same and all(torch.equal(a, b) for a, b in zip(results["host"], results["kernel"]))
            steps = int(results["kernel"][1].sum())
        lengths, outcome = results["kernel"][1], results["kernel"][2]
        med = {k: statistics.median(v) for k, v in seconds.items()}
        leg = {"batch": B, "episodes": E, "evaluation_steps": steps, "host_seconds": seconds["host"], "kernel_seconds": seconds["kernel"],
               "host_steps_per_s": [steps / s for s in seconds["host"]], "kernel_steps_per_s": [steps / s for s in seconds["kernel"]],
               "ratio_of_medians": med["host"] / med["kernel"], "same_results": bool(same),
               "mean_length": float(lengths.double().mean()), "longest_episode": int(lengths.max()),
               "time_limit_share": float(((outcome & 8) != 0).double().mean()), "success_share": float(((outcome & 4) != 0).double().mean())}
        legs.append(leg)
        say(f"B {B:5d} E {E}: {steps} evaluation steps (mean length {leg['mean_length']:.1f}, longest {leg['longest_episode']}, time limit "
            f"{100 * leg['time_limit_share']:.1f} %)   host " + " ".join(f"{1e3 * s:.1f}" for s in seconds["host"]) + " ms   in-kernel "
            + " ".join(f"{1e3 * s:.2f}" for s in seconds["kernel"]) + f" ms   x{leg['ratio_of_medians']:.1f}   host "
            + f"{steps / med['host']:.3e} steps/s, in-kernel {steps / med['kernel']:.3e} steps/s   same results: {same}")
    # ONE launch of the default launch_steps at the largest batch: four episodes per row, so that a row at the time limit makes every step
    B = legs[-1]["batch"]
    env = envs["kernel"]
    launch_ms = []
    for _ in range(args.rounds):
        from_the_start(env)
        progress = evaluate.new_progress(B, env.device)
        out = {name: torch.zeros(B, 4, dtype=dtype, device=env.device) for name, dtype in evaluate.OUTPUTS}
        dt, _ = timed(lambda: evaluate.launch_rays(env, theta, 4, evaluate.DEFAULT_LAUNCH_STEPS, progress, out, seed=SEED))
        launch_ms.append(1e3 * dt)
    most, made = int(progress["steps_done"].max()), int(progress["steps_done"].sum())
    say(f"one launch of launch_steps = {evaluate.DEFAULT_LAUNCH_STEPS} at B {B}, four episodes per row: "
        + " ".join(f"{ms:.2f}" for ms in launch_ms) + f" ms; the busiest row made {most} steps, all rows {made}")
    head = legs[-1]
    line = json.dumps({"metric": "greedy evaluation: environment steps/sec (act + auto-reset step + episode bookkeeping inside one launch)",
                       "value": statistics.median(head["kernel_steps_per_s"]), "unit": "env-steps/s", "n_gpus": 1,
                       "higher_is_better": True, "dtype": "f64 step, f32 policy", "data": "synthetic",
                       "config": {"workload": "scene 1 of tools/train_dqn.py, max_episode_steps 400, a fixed random theta, eps 0; both "
                                              "legs in one process, alternating", "batch_per_gpu": head["batch"], "episodes": E,
                                  "rounds": args.rounds, "launch_steps": evaluate.DEFAULT_LAUNCH_STEPS,
                                  "partner": "collect.act + env.step(auto_reset=True) + torch bookkeeping in the same run",
                                  "one_launch_ms": launch_ms, "one_launch_busiest_row_steps": most, "legs": legs}})
    say(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
