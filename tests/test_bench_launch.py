"""CPU: `python bench.py --gpus N` run DIRECTLY (no launcher, WORLD_SIZE unset) must start N rank processes itself
(one per GPU on a real node), reduce over them and report n_gpus = N; a mismatch between --gpus and WORLD_SIZE, or too
few devices, must fail loudly.  The solver is stubbed (MPCGPU_BENCH_STUB=1, gloo) -- this tests the launch and reduction
plumbing only; the JSON line says data = "stub"."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_bench_self_launches_two_ranks_when_run_without_a_launcher():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--batch", "64", "--cpu-seconds", "0", "--full"],
                       env=_env(MPCGPU_BENCH_BACKEND="gloo", MPCGPU_BENCH_STUB="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                             # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["data"] == "stub"
    assert len(line["per_rank_solves_per_s"]) == 2
    assert line["steps"] == 3 and line["warmup"] == 1 and line["scaling"] == "weak"
    # whole-job value = all ranks' problems / max-over-ranks time
    assert abs(line["value"] - 2 * 64 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]
    assert line["value"] <= sum(line["per_rank_solves_per_s"]) * (1 + 1e-9)
    assert line["config"]["convergent"]["value"] > 0 and line["config"]["avoidance"]["value"] > 0      # --full: side legs on every rank
    assert "ordered_perfect_hints" in line["config"] and "ordered" not in line["config"]
    assert "roofline" not in line and "cpu_baseline" not in line  # the stub measures nothing


def test_multi_rank_run_without_full_is_bounded_by_the_headline_leg():
    """An N-rank run reports the headline leg only (the side legs belong to the one-rank run, or to --full)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "64", "--cpu-seconds", "0"],
                       env=_env(MPCGPU_BENCH_BACKEND="gloo", MPCGPU_BENCH_STUB="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["n_gpus"] == 2 and line["value"] > 0
    for k in ("convergent", "avoidance", "batch_sweep", "closed_loop", "ordered_perfect_hints"):
        assert k not in line["config"], k


def test_one_rank_run_is_the_headline_leg_unless_full():
    """A plain one-rank run is the headline leg and nothing else; --full adds the side legs after it."""
    runs = {}
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "64"] + extra,
                           env=_env(MPCGPU_BENCH_STUB="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        runs[bool(extra)] = json.loads(lines[0])
    plain, full = runs[False], runs[True]
    for line in (plain, full):
        assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["data"] == "stub"
        assert abs(line["value"] - 64 * 2 / (line["ms_per_step"] * 2e-3)) < 1e-6 * line["value"]
    for k in ("convergent", "avoidance", "batch_sweep", "closed_loop", "ordered_perfect_hints", "other_stall_reading", "host_boundary"):
        assert k not in plain["config"], k
    assert full["config"]["convergent"]["value"] > 0 and full["config"]["avoidance"]["value"] > 0
    assert "ordered_perfect_hints" in full["config"]
    assert set(plain) == set(full) and set(plain["config"]) < set(full["config"])   # --full adds objects to config, nothing else


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--batch", "8"],
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MPCGPU_BENCH_STUB="1"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8"],
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MPCGPU_BENCH_STUB="1"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_bench_exits_non_zero_when_fewer_devices_than_gpus():
    import torch
    have = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(have + 2), "--batch", "8"],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr


def test_the_drivers_eight_rank_launch_is_rehearsed_with_stubbed_ranks():
    """The driver's command for the scaling run, word for word (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 8
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 8 --steps K --warmup W`), with the solver stubbed and gloo in place of
    RCCL: exit code 0, ONE JSON line, eight per-rank rates, no rank left behind in destroy_process_group, inside a minute."""
    import socket
    import time
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1",
                        "--batch", "64"],
                       env=_env(MPCGPU_BENCH_BACKEND="gloo", MPCGPU_BENCH_STUB="1", OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=280)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["rccl_ranks"] == 8 and len(line["per_rank_solves_per_s"]) == 8
    assert line["steps"] == 3 and line["warmup"] == 1 and line["scaling"] == "weak" and line["higher_is_better"] is True
    assert abs(line["value"] - 8 * 64 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]
    assert line["config"]["parallelism"] == "shard8" and line["psi_evals_per_s"] > 0
    for k in ("convergent", "avoidance", "batch_sweep", "closed_loop", "ordered_perfect_hints", "metric_batch"):
        assert k not in line["config"], k             # an N-rank run is the headline leg and nothing else
    assert "roofline" not in line and "cpu_baseline" not in line
    assert wall < 120, wall


def test_cpu_baseline_reports_parity_of_the_run_on_its_sample():
    """bench.py's cpu_baseline leg times the oracle AND uses its answers as the checker of the run: handed the control sequences
    of the timed launches for the same problems it reports the converged pairs, their largest difference and the agreement on
    which problems converge.  (CPU: the oracle's own answers stand in for the GPU's, one of them moved by 1e-6.)"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    import oracle
    from conftest import make_cfg
    from trajtrack_mpcndqn_rlboost_amd import scenes
    cfg = make_cfg(20, solver_max_inner_iterations=120, solver_max_outer_iterations=4)
    p = scenes.make_family(cfg, 64, "passing", n_dyn=4, seed=3)["p"]
    u, _, res, _ = oracle.solve_batch(oracle.OracleConfig.from_dict(cfg.solver_dict()), p)
    st = np.asarray(res["status"]).copy()
    conv = np.flatnonzero(st == 0)
    assert len(conv) >= 2 and len(conv) < 64            # the sample holds converged AND cap-limited solves
    u_gpu = np.array(u, copy=True)
    u_gpu[conv[0], 3] += 1e-6
    out = bench.cpu_baseline(cfg, p, 0.2, gpu_u=u_gpu, gpu_status=st)
    par = out["parity_on_sample"]
    S = par["problems"]
    assert out["kind"] == "port" and out["value"] > 0 and 1 <= S <= 64
    n_conv = int(np.sum(st[:S] == 0))
    assert par["converged_on_both_sides"] == n_conv and par["same_converged_or_not"] == 1.0 and par["tolerance"] == 1e-3
    if conv[0] < S:
        assert abs(par["max_abs_du_on_them"] - 1e-6) < 1e-12


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the arrays of the headline leg's last timed step, one float64 .npy each, with --steps timed steps."""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "64",
                        "--cpu-seconds", "0", "--dump-outputs", str(d)],
                       env=_env(MPCGPU_BENCH_STUB="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    names = sorted(f.name for f in d.iterdir())
    assert names == sorted(f"{k}.npy" for k in ("u", "cost", "status", "inner_it", "outer_it", "f2norm")), names
    u = np.load(d / "u.npy")
    assert u.dtype == np.float64 and u.shape == (64, 40) and not u.any()          # what the stub solver wrote
    assert np.array_equal(np.load(d / "inner_it.npy"), np.full(64, 7.0))
    assert np.array_equal(np.load(d / "status.npy"), np.ones(64))


def test_dump_outputs_samples_the_same_rows_when_over_budget(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    B = 1000
    out = {"u": np.arange(B * 40, dtype=np.float64).reshape(B, 40), "status": np.arange(B, dtype=np.int32)}
    budget = 100 * 8 * 41 + 4096 * 3 + 100 * 8
    names = bench.dump_outputs(str(tmp_path), out, budget=budget)
    assert names == ["sample_rows", "status", "u"]
    rows = np.load(tmp_path / "sample_rows.npy")
    assert len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "status.npy"), rows)
    assert np.array_equal(np.load(tmp_path / "u.npy")[:, 0], rows * 40)
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= budget
    bench.dump_outputs(str(tmp_path / "again"), out, budget=budget)
    assert np.array_equal(np.load(tmp_path / "again" / "sample_rows.npy"), rows)     # fixed seed: the same sample every run
