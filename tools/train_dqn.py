#!/usr/bin/env python3
"""DQN training on the batched HIP environment (BASELINE.json config 5 in miniature, one GPU per process).

    python tools/train_dqn.py [--gpus N] [--envs 4096] [--timesteps 4000000] [--gradient-steps 16] [--batch-size 256]
                              [--save DIR] [--resume DIR/checkpoint.pt] [--checkpoint-every STEPS]
                              [--images] [--fresh-maps] [--per] [--buffer-size N] [--graph | --fused [--per-in-kernel]]
                              [--collect-in-kernel | --fresh-maps --collect-turnover]
                              [--eval-freq STEPS [--eval-envs M] [--eval-episodes E]]

`--images` trains dqn.ImageQNetwork on the image environment (rl_env.BatchedImgsEnv); with `--fresh-maps` every episode of it
starts on a new random map too (map_turnover=True, capacity map_stream.DYNAMIC_CAPACITY, stream seed + rank).

`--fused` runs the update as the fused HIP kernel (dqn_fused.FusedDqnTrainer; ray network, batch size at most
256): with uniform replay and one rank a whole update round is one launch, which makes `--gradient-steps -1` -- one gradient
step per collected transition, the reference's setting -- affordable.  With `--per` the round is one launch per step around the
tree's kernels unless `--per-in-kernel` moves sample, update and re-prioritisation into the launch as well.

`--collect-in-kernel` (ray environment without --fresh-maps, one or several GPUs) collects the steps of a round -- act, auto-reset
step, buffer rows, episode returns -- inside ONE launch of the step kernel (collect.collect_rays) instead of some
forty launches per step; exploration then draws from a counter stream of its own.

`--fresh-maps --collect-turnover` (ray environment) does the same on the two-record table of the map stream
(collect_fresh.collect_rays_fresh): a row whose episode ends inside a launch moves to its new map there; the
refill of the spares follows a launch, never splits it.

`--eval-freq STEPS` (ray environment) is the reference's EvalCallback (src/test_block_rl.py:65-99) on the device: every STEPS
environment steps the greedy policy plays `--eval-episodes` episodes on each of `--eval-envs` maps of a separate environment
inside the step kernel (evaluate.EvalCallback).  best_model.pt is then chosen by the mean evaluation return,
`--save DIR` also receives evaluations.npz (timesteps, results, ep_lengths, successes) and, for `--resume`, the callback's state
in eval_callback.pt beside the checkpoint.  The training run itself is the run without the flag, bit for bit.

`--save DIR` writes what the reference's run leaves behind (src/test_block_rl.py:73-76,89-96: EvalCallback's best_model and
model.save's final_model) -- best_model.pt whenever the mean return of a progress window improves, final_model.pt at the end --
plus checkpoint.pt (network, target network, Adam moments, counters, generator, replay buffer, environment state) every
`--checkpoint-every` environment steps; `--resume` continues such a checkpoint exactly where it stopped (rank 0's files; in a
multi-rank run every rank restores its own `checkpoint.rank<r>.pt`).

`--gpus N` without a launcher starts the N ranks itself (fresh child processes of torch.distributed.run, before anything in
this process touches a GPU); it exits non-zero when fewer than N devices are visible.  Rank 0 ends with ONE JSON line
(environment steps/s and Q-network updates/s of the whole job, ranks, backend; `double_q` says whether they are double-Q updates).

Every environment is scene 1 of the reference (src/pkg_dqn/utils/map.py:292-305) with the 'medium' box and a periodic
obstacle, start pose jittered per environment; the reference path is the straight line start -> goal (an input; the
reference gets it from A*).  Under torch.distributed (torchrun, backend nccl = RCCL) every rank trains on its own
environments and the gradients are summed by one flat all-reduce per update.  Prints throughput and the return curve."""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
map_stream = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.map_stream")
path_plan = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.path_plan")
dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")


def scene(rng):
    y0 = 3.5 + rng.uniform(-1.0, 1.0)
    th = rng.uniform(-0.5, 0.5)
    return rl_env.make_map(
        boundary=[(0.0, 0.0), (16.0, 0.0), (16.0, 10.0), (0.0, 10.0)],
        static=[[(0.0, 1.5), (0.0, 1.6), (9.0, 1.6), (9.0, 1.5)], [(0.0, 8.4), (0.0, 8.5), (9.0, 8.5), (9.0, 8.4)],
                [(11.0, 1.5), (11.0, 1.6), (16.0, 1.6), (16.0, 1.5)], [(11.0, 8.4), (11.0, 8.5), (16.0, 8.5), (16.0, 8.4)],
                [(7.2, 2.8), (7.2, 4.2), (8.8, 4.2), (8.8, 2.8)]],
        dynamic=[dict(p1=(10.0, 1.0), p2=(10.0, 9.0), freq=0.2, rx=0.8, ry=0.8, angle=0.0, corners=20)],
        start=[0.6, y0, th, 0.0, 0.0], goal=[15.4, 3.5], path=[(0.6, y0), (6.4, 5.4), (9.6, 5.4), (15.4, 3.5)])


def fresh_start_maps(n: int, device: int):
    """The maps the environments of --fresh-maps start on: a handful of host-built generate_map_dynamic maps, repeated (every row
    moves to a map of its own at its first episode end)."""
    specs = [map_stream.spec_of(2 ** 40, b) for b in range(16)]
    paths, status = path_plan.plan_reference_paths(specs, device=device)
    maps = [rl_env.make_map(path=p, **s) for s, p, st in zip(specs, paths, status) if st == 0][:4]
    return [maps[i % len(maps)] for i in range(n)]


def self_launch(gpus: int) -> int:
    if torch.cuda.device_count() < gpus:
        print(f"train_dqn.py: --gpus {gpus} but only {torch.cuda.device_count()} GPU(s) visible", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--timesteps", type=int, default=4_000_000)
    ap.add_argument("--gradient-steps", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--double-q", action="store_true")
    ap.add_argument("--per", action="store_true", help="prioritized experience replay (device-resident sum tree; the reference's 'per': True)")
    ap.add_argument("--graph", action="store_true", help="replay the update from captured HIP graphs (multi-rank: two graphs around the all-reduce)")
    ap.add_argument("--fused", action="store_true",
                    help="the update as one fused HIP kernel (ray network only); with it --gradient-steps -1 is the reference's ratio")
    ap.add_argument("--per-in-kernel", action="store_true",
                    help="with --fused --per on one GPU: sample, update and re-prioritise inside the launch, one launch per update round")
    ap.add_argument("--collect-in-kernel", action="store_true",
                    help="collect the steps of a round inside one launch of the step kernel (ray environment, not with --fresh-maps)")
    ap.add_argument("--collect-turnover", action="store_true",
                    help="with --fresh-maps (ray environment): collect inside the launch on the two-record table of the map stream")
    ap.add_argument("--save", default=None, help="directory for best_model.pt / final_model.pt / checkpoint.pt")
    ap.add_argument("--resume", default=None, help="checkpoint.pt of an earlier run with the same arguments")
    ap.add_argument("--checkpoint-every", type=int, default=0, help="environment steps between checkpoints (0: only at the end)")
    ap.add_argument("--fresh-maps", action="store_true",
                    help="a new random map per episode, drawn and planned on the device (generate_map_dynamic; stream seed + rank)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the map stream of --fresh-maps")
    ap.add_argument("--images", action="store_true",
                    help="train dqn.ImageQNetwork on the image environment (BatchedImgsEnv); combines with --fresh-maps and --per")
    ap.add_argument("--buffer-size", type=int, default=None,
                    help="replay transitions (default 2000000; 200000 with --images, whose transitions hold two uint8 images)")
    ap.add_argument("--eval-freq", type=int, default=0,
                    help="environment steps between greedy evaluations on a separate environment (evaluate.EvalCallback); 0: off")
    ap.add_argument("--eval-envs", type=int, default=64, help="maps of the evaluation environment")
    ap.add_argument("--eval-episodes", type=int, default=1, help="evaluation episodes per map")
    args = ap.parse_args(argv)
    if args.eval_freq < 0 or (args.eval_freq and (args.eval_envs < 1 or args.eval_episodes < 1)):
        ap.error("--eval-freq must not be negative; --eval-envs and --eval-episodes must be at least 1")
    if args.eval_freq and args.images:
        ap.error("--eval-freq evaluates inside the step kernel of the ray environment: not with --images")
    if args.per_in_kernel and not (args.fused and args.per):
        ap.error("--per-in-kernel is the prioritized form of the fused K-step launch: it needs --fused and --per")
    if args.per_in_kernel and args.gpus > 1:
        ap.error("--per-in-kernel is the one-GPU path: several ranks update step by step around the all-reduce")
    if args.collect_in_kernel and (args.images or args.fresh_maps):
        ap.error("--collect-in-kernel is built for the ray environment on one record table: not with --images or --fresh-maps "
                 "(--fresh-maps --collect-turnover collects inside the launch on the two-record table)")
    if args.collect_turnover and (args.images or not args.fresh_maps):
        ap.error("--collect-turnover is collection inside the launch on the two-record table: it needs --fresh-maps and the ray "
                 "environment (not --images)")
    return args


def main():
    args = parse_args()
    if os.environ.get("WORLD_SIZE") is None and args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus and (world > 1 or args.gpus > 1):
        sys.exit(f"train_dqn.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    rng = np.random.default_rng(100 + rank)
    torch.manual_seed(0)
    # --images: the image environment; DqnLearner then builds dqn.ImageQNetwork and keeps the images as uint8 in the buffer
    if args.fresh_maps:
        kind = dict(map_turnover=True) if args.images else {}
        env = (rl_env.BatchedImgsEnv if args.images else rl_env.BatchedRaysEnv)(
            fresh_start_maps(args.envs, local), device=local, max_episode_steps=400, capacity=map_stream.DYNAMIC_CAPACITY, **kind)
        env.enable_fresh_maps(seed=args.seed + rank)
    else:
        env = (rl_env.BatchedImgsEnv if args.images else rl_env.BatchedRaysEnv)(
            [scene(rng) for _ in range(args.envs)], device=local, max_episode_steps=400)
    if args.images and args.graph:
        sys.exit("train_dqn.py: --graph is not built for --images (the image update runs eagerly)")
    if args.fused and (args.images or args.graph):
        sys.exit("train_dqn.py: --fused is built for the ray network and excludes --graph")
    trainer = dqn_train.make_trainer(env, fused=args.fused, device=f"cuda:{local}", double_q=args.double_q, lr=1e-3)
    buffer_size = args.buffer_size or (200_000 if args.images else 2_000_000)
    learner = dqn_train.DqnLearner(env, trainer, buffer_size=buffer_size, learning_starts=4 * args.envs,
                                   batch_size=args.batch_size, train_freq=4, gradient_steps=args.gradient_steps,
                                   target_update_interval=200_000, exploration_fraction=0.3, use_graph=args.graph,
                                   track_episodes=False, per=args.per, fused=args.fused, per_in_kernel=args.per_in_kernel,
                                   collect_in_kernel=args.collect_in_kernel or args.collect_turnover,
                                   collect_turnover=args.collect_turnover)
    ck_name = "checkpoint.pt" if rank == 0 else f"checkpoint.rank{rank}.pt"
    eval_cb, eval_name = None, "eval_callback.pt" if rank == 0 else f"eval_callback.rank{rank}.pt"
    if args.eval_freq:
        # EvalCallback of the reference's run: greedy episodes on maps of their own (a generator of its own, so the training maps
        # are the ones of a run without it), every rank on its own environment; rank 0 writes best_model.pt and evaluations.npz
        evaluate = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.evaluate")
        eval_rng = np.random.default_rng(10_000 + rank)
        eval_env = rl_env.BatchedRaysEnv([scene(eval_rng) for _ in range(args.eval_envs)], device=local, max_episode_steps=400)
        files = args.save if rank == 0 else None
        eval_cb = evaluate.EvalCallback(eval_env, args.eval_freq, n_eval_episodes=args.eval_episodes, best_model_save_path=files,
                                        log_path=files, seed=0x45564131 + rank)
    if args.resume:
        learner.load(args.resume if rank == 0 else os.path.join(os.path.dirname(args.resume), ck_name))
        if eval_cb is not None and os.path.exists(os.path.join(os.path.dirname(args.resume), eval_name)):
            eval_cb.load_state_dict(torch.load(os.path.join(os.path.dirname(args.resume), eval_name), weights_only=True))
        if rank == 0:
            print(f"  resumed at {learner.num_timesteps} environment steps, {learner.trainer.num_updates} updates", flush=True)
    if args.save:
        os.makedirs(args.save, exist_ok=True)
    marks, t0 = [], time.perf_counter()
    best = [-float("inf")]

    def progress(lr):
        if lr.num_timesteps // (args.timesteps // 10) > len(marks):
            n, r, ok = float(lr.ep_count), float(lr.ep_return_sum), float(lr.ep_success_sum)      # one sync per mark
            pn, pr, pok = marks[-1][4:] if marks else (0.0, 0.0, 0.0)
            dn = max(n - pn, 1.0)
            marks.append((lr.num_timesteps, (r - pr) / dn, (ok - pok) / dn, time.perf_counter() - t0, n, r, ok))
            if rank == 0:
                print(f"  {marks[-1][0]:>9d} steps  mean return {marks[-1][1]:8.2f}  success {marks[-1][2]:.2f}  {marks[-1][3]:6.1f} s", flush=True)
                if args.save and eval_cb is None and marks[-1][1] > best[0]:       # EvalCallback(best_model_save_path=...)
                    best[0] = marks[-1][1]
                    learner.save_model(os.path.join(args.save, "best_model.pt"))

    def both(lr):
        progress(lr)
        before = eval_cb.n_evaluations
        eval_cb(lr)
        if rank == 0 and eval_cb.n_evaluations != before:
            print(f"  {lr.num_timesteps:>9d} steps  evaluation {eval_cb.n_evaluations}: mean return {eval_cb.last_mean_reward:8.2f} "
                  f"(best {eval_cb.best_mean_reward:.2f}), success {float(np.mean(eval_cb.successes[-1])):.2f}, "
                  f"mean length {float(np.mean(eval_cb.ep_lengths[-1])):.1f}", flush=True)

    callback = progress if eval_cb is None else both

    def checkpoint():
        learner.save(os.path.join(args.save, ck_name))
        if eval_cb is not None:
            torch.save(eval_cb.state_dict(), os.path.join(args.save, eval_name))

    if args.save and args.checkpoint_every > 0:
        stats = None
        while learner.num_timesteps < args.timesteps:
            stats = learner.learn(args.timesteps, callback=callback, stop_at=learner.num_timesteps + args.checkpoint_every)
            checkpoint()
    else:
        stats = learner.learn(args.timesteps, callback=callback)
    if args.save:
        checkpoint()
        if rank == 0:
            learner.save_model(os.path.join(args.save, "final_model.pt"))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rank == 0:
        print(f"envs/rank {args.envs} x ranks {world}: {world * stats['timesteps'] / dt:.3e} environment steps/s incl. "
              f"{stats['updates']} updates of batch {args.batch_size} ({stats['updates'] / dt:.0f} updates/s), "
              f"episodes {stats['episodes']}, final mean return {stats['mean_return']:.2f}, success rate {stats['success_rate']:.2f}")
        print(json.dumps({"metric": "DQN online training: environment steps/s (batched HIP environment + "
                                    + ("double-Q" if args.double_q else "DQN") + " updates)",
                          "value": world * stats["timesteps"] / dt, "unit": "environment steps/s", "n_gpus": world,
                          "rccl_ranks": dist.get_world_size() if world > 1 else 1, "backend": "nccl" if world > 1 else None,
                          "updates_per_s": stats["updates"] / dt, "gradient_all_reduce_floats": 1177 if world > 1 else 0,
                          "update_path": ("fused HIP kernels around one flat RCCL all-reduce" if world > 1 else
                                          "fused HIP kernel with the sum tree inside, one launch per update round" if args.per_in_kernel else
                                          "fused HIP kernel, one launch per step" if args.per else
                                          "fused HIP kernel, one launch per update round") if args.fused else "two HIP graphs around one flat RCCL all-reduce" if (args.graph and world > 1) else
                                         ("one HIP graph" if args.graph else "eager"),
                          "config": {"workload": "BASELINE.json config 5 (scene 1, medium box, periodic obstacle)",
                                     "envs_per_gpu": args.envs, "timesteps_per_gpu": int(stats["timesteps"]),
                                     "batch_size": args.batch_size, "gradient_steps": args.gradient_steps, "double_q": bool(args.double_q),
                                     "per": bool(args.per), "images": bool(args.images), "fresh_maps": bool(args.fresh_maps),
                                     "collect_in_kernel": bool(args.collect_in_kernel),
                                     "collect_turnover": bool(args.collect_turnover),
                                     "eval_freq": args.eval_freq, "evaluations": eval_cb.n_evaluations if eval_cb else 0,
                                     "buffer_size": buffer_size},
                          "success_rate": stats["success_rate"], "mean_return": stats["mean_return"]}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
