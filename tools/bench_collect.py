#!/usr/bin/env python3
"""Environment steps per second of pure collection: ``DqnLearner`` as it is against ``collect_in_kernel=True``.

    python tools/bench_collect.py [--batches 256,4096] [--train-freqs 4,16,64] [--steps K] [--warmup W] [--rounds 3]
                                  [--fresh-maps [--refill-every 16] [--stale-scan 4,16,64 [--run-steps 2000]]]

``learning_starts`` lies above the run, so a round of ``learn`` is its ``train_freq`` environment steps and nothing else: some
forty launches per step on the host-driven path, one launch per round with ``collect_in_kernel``.  Both learners live in ONE
process on environments of their own (scene 1 of tools/train_dqn.py, ``max_episode_steps`` 400, fused trainer,
``track_episodes=False``) and take turns: host, kernel, host, kernel, ... for ``--rounds`` rounds of ``--steps`` environment
steps each (a multiple of every train_freq), every round timed between two device synchronisations and written out.
Prints one line per (batch, train_freq) and ends with ONE JSON line in the shape of tools/bench_env.py; its value is the
in-kernel rate at the largest batch and the smallest train_freq, its config holds every round of both legs.

``--fresh-maps``: both legs on an ``enable_fresh_maps(refill_every=--refill-every)`` environment (the start maps of
tools/train_dqn.py --fresh-maps), ``DqnLearner`` as it is against ``collect_turnover=True`` with its default launch size; every leg
also records ``loaded`` and ``stale`` of both environments.  ``--stale-scan 4,16,64`` first prints, for each launch size, the
share of stale resets in ``--run-steps`` steps of random actions (eps = 1) at the largest batch: the rule that chooses
``collect_fresh.DEFAULT_LAUNCH_STEPS``."""
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
dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
train_dqn = importlib.import_module("tools.train_dqn")


_MAPS = {}


def fresh_env(B: int, refill_every: int):
    if ("fresh", B) not in _MAPS:
        _MAPS[("fresh", B)] = train_dqn.fresh_start_maps(B, 0)
    env = rl_env.BatchedRaysEnv(_MAPS[("fresh", B)], max_episode_steps=400, capacity=train_dqn.map_stream.DYNAMIC_CAPACITY)
    env.enable_fresh_maps(seed=0, refill_every=refill_every)
    return env


def make_learner(B: int, train_freq: int, in_kernel: bool, refill_every: int = 0):
    """``refill_every`` > 0: the environment of --fresh-maps, and ``in_kernel`` means ``collect_turnover=True``."""
    if refill_every:
        env = fresh_env(B, refill_every)
    else:
        if B not in _MAPS:       # the same maps for every learner of this batch size
            rng = np.random.default_rng(100)
            _MAPS[B] = [train_dqn.scene(rng) for _ in range(B)]
        env = rl_env.BatchedRaysEnv(_MAPS[B], max_episode_steps=400)
    torch.manual_seed(0)
    return dqn_train.DqnLearner(env, buffer_size=max(2 * 64 * B, 1 << 16), learning_starts=10 ** 12, train_freq=train_freq,
                                target_update_interval=200_000, exploration_fraction=0.3, track_episodes=False, fused=True,
                                collect_in_kernel=in_kernel, collect_turnover=in_kernel and refill_every > 0)


def stale_scan(B: int, refill_every: int, launch_steps, run_steps: int):
    """Share of stale resets in ``run_steps`` steps of random actions (eps = 1) per launch size, one JSON line each."""
    collect_fresh = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.collect_fresh")
    for T in launch_steps:
        env = fresh_env(B, refill_every)
        env.reset()
        buf = dqn_train.ReplayBuffer(2 * 64 * B, 46, env.device)
        theta = torch.zeros(1177, dtype=torch.float32, device=env.device)
        ep = torch.zeros(B, dtype=torch.float64, device=env.device)
        for k in range(run_steps // T):
            collect_fresh.collect_rays_fresh(env, theta, buf, [1.0] * T, 1, k * T, ep)
        torch.cuda.synchronize()
        loaded, stale = float(env.loaded.sum()), float(env.stale.sum())
        print(json.dumps({"metric": "map turnover inside the launch under random actions", "batch": B, "refill_every": refill_every,
                          "launch_steps": T, "run_steps": run_steps // T * T, "loaded": loaded, "stale": stale,
                          "stale_share": stale / max(loaded + stale, 1.0)}), flush=True)
        del env, buf
        torch.cuda.empty_cache()


def timed(learner, total: int, steps: int) -> float:
    """``steps`` more environment steps of ``learner`` -> environment steps per second (B rows each)."""
    B = learner.env.B
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    learner.learn(total, stop_at=learner.num_timesteps + steps * B)
    torch.cuda.synchronize()
    return steps * B / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--train-freqs", default="4,16,64")
    ap.add_argument("--steps", type=int, default=256, help="environment steps of one timed round (a multiple of every train_freq)")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fresh-maps", action="store_true", help="both legs on the map stream; the in-kernel leg is collect_turnover=True")
    ap.add_argument("--refill-every", type=int, default=16)
    ap.add_argument("--stale-scan", default="", help="with --fresh-maps: launch sizes whose stale share is printed first, e.g. 4,16,64")
    ap.add_argument("--run-steps", type=int, default=2000)
    args = ap.parse_args()
    every = args.refill_every if args.fresh_maps else 0
    batches = [int(b) for b in args.batches.split(",")]
    freqs = [int(f) for f in args.train_freqs.split(",")]
    if any(args.steps % f or args.warmup % f for f in freqs):
        ap.error("--steps and --warmup must be multiples of every train_freq")
    if args.fresh_maps and args.stale_scan:
        stale_scan(max(batches), every, [int(t) for t in args.stale_scan.split(",")], args.run_steps)
    legs = []
    for B in batches:
        for tf in freqs:
            total = 20 * (args.warmup + args.rounds * args.steps) * B          # the run stays in the first 5 % of the schedule
            pair = {"host": make_learner(B, tf, False, every), "kernel": make_learner(B, tf, True, every)}
            rates = {"host": [], "kernel": []}
            for name, lr in pair.items():
                timed(lr, total, args.warmup)
            for _ in range(args.rounds):
                for name, lr in pair.items():
                    rates[name].append(timed(lr, total, args.steps))
            med = {k: statistics.median(v) for k, v in rates.items()}
            spread = max((max(v) - min(v)) / statistics.median(v) for v in rates.values())
            leg = {"batch": B, "train_freq": tf, "host_env_steps_per_s": rates["host"], "kernel_env_steps_per_s": rates["kernel"],
                   "ratio_of_medians": med["kernel"] / med["host"], "largest_round_to_round_spread": spread,
                   "buffer_rows": [lr.buffer.size for lr in pair.values()]}
            if every:
                leg.update(refill_every=every, launch_steps=pair["kernel"].collect_launch_steps,
                           loaded=[int(lr.env.loaded.sum()) for lr in pair.values()], stale=[int(lr.env.stale.sum()) for lr in pair.values()])
            legs.append(leg)
            print(f"B {B:5d} train_freq {tf:2d}: host " + " ".join(f"{r:.3e}" for r in rates["host"]) + "   in-kernel "
                  + " ".join(f"{r:.3e}" for r in rates["kernel"]) + f"   x{leg['ratio_of_medians']:.2f} (spread {100 * spread:.1f} %)"
                  + (f"   loaded {leg['loaded']} stale {leg['stale']}" if every else ""), flush=True)
            del pair
            torch.cuda.empty_cache()
    head = max(legs, key=lambda g: (g["batch"], -g["train_freq"]))
    print(json.dumps({"metric": "DQN collection: environment steps/sec (act + auto-reset step + replay rows inside one launch)",
                      "value": statistics.median(head["kernel_env_steps_per_s"]), "unit": "env-steps/s", "n_gpus": 1,
                      "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "dtype": "f64 step, f32 policy",
                      "data": "synthetic",
                      "config": {"workload": ("the map stream of tools/train_dqn.py --fresh-maps" if every else "scene 1 of tools/train_dqn.py")
                                             + ", fused trainer, learning_starts above the run, "
                                             "track_episodes=False; both legs in one process, alternating",
                                 "batch_per_gpu": head["batch"], "train_freq": head["train_freq"], "rounds": args.rounds,
                                 "fresh_maps": bool(every),
                                 "partner": "DqnLearner(collect_in_kernel=False) in the same run", "legs": legs}}), flush=True)


if __name__ == "__main__":
    main()
