#!/usr/bin/env python3
"""Golden trace of the reference's own prioritized replay buffer.

Run in the build container only (needs /root/reference):   python tests/golden/make_per_fixture.py
                                                           python tests/golden/make_per_fixture.py NAME   (a row of SETTINGS)

The reference's ``PerReplayBuffer`` (src/pkg_dqn/utils/per_dqn.py:25-187) is loaded from the reference tree at run time
and executed on a seeded schedule of adds, samples and re-prioritizations.  stable_baselines3 and gym are not installed;
the class needs of them only a base class that keeps ``buffer_size``, ``pos`` and ``full``, so those modules are stubbed
(as make_dqn_fixtures.py stubs shapely).  ``np.random.uniform`` is replaced by a recording function fed from a seeded
generator (numpy's own formula, low + (high - low) * u), so the trace holds the ``u`` of every draw.

Schedule: capacity 300 (not a power of two: leaves on two depths), update_max_freq 100 (a multiple of the rows per
call, where the buffer here reads max_p at the same rows as the reference), 60 calls of one row, then 180 calls of four rows
(the ring wraps twice); after every call one sample of 32 and the re-prioritization of its rows, with TD errors that are
float32 values (the device takes float32).  Recorded per step: rows added, max_p, the u, the returned indices and
weights, the TD errors; every 20 steps the leaves, tree[0] and the reference's own drift |tree[0] - fsum(leaves)| /
tree[0].  ``tolerance`` = ten times the largest drift: how far the reference is from its own exact sum, with a margin.
A draw is DECIDABLE when its s lies further than tolerance * tree[0] from every leaf boundary of the exact prefix sums;
the script refuses to write a trace with an undecidable draw (change SEED if it ever trips).
Only data is written: per_trace.npz, or the file of the named row of SETTINGS -- the same schedule and SEED at other settings
of the buffer (the ones most users take from the literature, and the corners alpha = 1 / beta = 0 / initial_priority != 1).
"""
import importlib.util
import io
import math
import os
import sys
import types
import zipfile
from fractions import Fraction

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016
CAPACITY, FREQ, N_SAMPLE = 300, 100, 32
SINGLE_CALLS, QUAD_CALLS, CHECK_EVERY = 60, 180, 20
# name -> (file, keyword arguments of the reference's PerReplayBuffer); "default" passes none, as the script always did
SETTINGS = {
    "default": ("per_trace.npz", {}),
    "a06_b10_e1e-6": ("per_trace_a06_b10_e1e-6.npz", dict(alpha=0.6, beta=1.0, epsilon=1e-6)),
    "a10_b00_e1e-2_p25": ("per_trace_a10_b00_e1e-2_p25.npz", dict(alpha=1.0, beta=0.0, epsilon=1e-2, initial_priority=2.5)),
}


class _DictReplayBuffer:
    """What PerReplayBuffer uses of SB3's DictReplayBuffer: the ring position."""

    def __init__(self, buffer_size, observation_space=None, action_space=None, device="cpu", n_envs=1,
                 optimize_memory_usage=False, handle_timeout_termination=True):
        self.buffer_size, self.pos, self.full = buffer_size, 0, False

    def add(self, obs, next_obs, action, reward, done, infos):
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full, self.pos = True, 0

    def _get_samples(self, batch_inds, env=None):
        return (None, None, None, None, None)

    def reset(self):
        self.pos, self.full = 0, False


def _stub(name, **members):
    mod = types.ModuleType(name)
    mod.__dict__.update(members)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def load_reference_class():
    anything = type("Anything", (), {})
    _stub("gym", spaces=_stub("gym.spaces", Space=anything))
    _stub("stable_baselines3", DQN=anything)
    _stub("stable_baselines3.common")
    _stub("stable_baselines3.common.buffers", DictReplayBuffer=_DictReplayBuffer)
    _stub("stable_baselines3.common.policies", BasePolicy=anything)
    _stub("stable_baselines3.common.type_aliases", GymEnv=anything, Schedule=anything, TensorDict=dict)
    _stub("stable_baselines3.dqn")
    _stub("stable_baselines3.dqn.policies", CnnPolicy=anything, DQNPolicy=anything, MlpPolicy=anything,
          MultiInputPolicy=anything)
    _stub("stable_baselines3.common.vec_env", VecNormalize=anything)
    _stub("ref_utils")
    for name in ("type_aliases", "per_dqn"):
        spec = importlib.util.spec_from_file_location(f"ref_utils.{name}", os.path.join(REF, "src/pkg_dqn/utils", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_utils.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["ref_utils.per_dqn"].PerReplayBuffer


def leaf_order(capacity):
    """Tree indices of the leaves from left to right: the deepest depth first, then the leaves one depth up."""
    split = (1 << int(math.floor(math.log2(2 * capacity - 1)))) - 1
    return np.concatenate([np.arange(split, 2 * capacity - 1), np.arange(capacity - 1, split)])


def savez_deterministic(path, **arrays):
    """np.savez_compressed without the wall-clock time stamps in the zip headers: reruns give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(name="default"):
    file, settings = SETTINGS[name]
    PerReplayBuffer = load_reference_class()
    rng = np.random.default_rng(SEED)
    drawn = []

    def recording_uniform(low, high):
        u = rng.random()
        drawn.append(u)
        return low + (high - low) * u

    np.random.uniform = recording_uniform
    rows_of = [1] * SINGLE_CALLS + [4] * QUAD_CALLS
    S = len(rows_of)
    order = leaf_order(CAPACITY)
    out = dict(rows=np.array(rows_of), pos=np.zeros(S, np.int64), n_entries=np.zeros(S, np.int64), max_p=np.zeros(S),
               u=np.zeros((S, N_SAMPLE)), indices=np.zeros((S, N_SAMPLE), np.int64), weights=np.zeros((S, N_SAMPLE)),
               td=np.zeros((S, N_SAMPLE), np.float32), margin=np.zeros(S))
    ck_step, ck_leaves, ck_total, ck_drift = [], [], [], []
    repeated = 0
    for step, rows in enumerate(rows_of):
        buf = PerReplayBuffer(CAPACITY, None, None, "cpu", n_envs=rows, update_max_freq=FREQ, **settings) if step == 0 else buf
        buf._n_envs = rows
        out["pos"][step] = buf.pos
        empty = {"x": np.zeros((rows, 1))}
        buf.add(empty, empty, np.zeros((rows, 1)), np.zeros(rows), np.zeros(rows), [{}] * rows)
        out["max_p"][step] = buf.max_p
        out["n_entries"][step] = buf.buffer_size if buf.full else buf.pos
        # exact leaf boundaries (left-to-right leaf order) before the draw
        bounds, acc = [], Fraction(0)
        for v in buf.tree[order]:
            acc += Fraction(float(v))
            bounds.append(acc)
        del drawn[:]
        sample = buf.sample(N_SAMPLE)
        assert len(drawn) == N_SAMPLE, "the reference retried the draw (a zero leaf): pick another SEED"
        indices, weights = sample[5], sample[6]
        total = buf.tree[0]
        segment = total / N_SAMPLE
        margin = math.inf
        for i, u in enumerate(drawn):
            a, b = segment * i, segment * (i + 1)
            s = Fraction(float(a + (b - a) * u))
            margin = min(margin, float(min(abs(s - bd) for bd in bounds)) / total)
        td = (rng.standard_normal(N_SAMPLE) * np.exp(rng.uniform(-3.0, 1.5))).astype(np.float32)
        for i in range(N_SAMPLE):               # PerDQN.train: one call per sampled row, in row order
            buf.update_priority(int(indices[i]), float(td[i]))
        repeated += N_SAMPLE - len(set(indices.tolist()))
        out["u"][step], out["indices"][step], out["weights"][step], out["td"][step] = drawn, indices, weights, td
        out["margin"][step] = margin
        if (step + 1) % CHECK_EVERY == 0 or step == S - 1:
            leaves = buf.tree[CAPACITY - 1:].copy()
            ck_step.append(step); ck_leaves.append(leaves); ck_total.append(buf.tree[0])
            ck_drift.append(abs(buf.tree[0] - math.fsum(leaves)) / buf.tree[0])
    tolerance = 10.0 * max(ck_drift)
    assert tolerance > 0.0
    assert out["margin"].min() > tolerance, ("undecidable draw: change SEED", out["margin"].min(), tolerance)
    assert repeated > 0, "no repeated index in any sample: the last-row-wins rule is not exercised"
    savez_deterministic(os.path.join(HERE, file), capacity=CAPACITY, update_max_freq=FREQ, alpha=buf.alpha,
                        beta=buf.beta, epsilon=buf.epsilon, initial_priority=float(buf.initial_priority),
                        ck_step=np.array(ck_step), ck_leaves=np.array(ck_leaves), ck_total=np.array(ck_total),
                        ck_drift=np.array(ck_drift), tolerance=tolerance, **out)
    print(f"{file}: {S} steps, {S * N_SAMPLE} draws, {repeated} repeated indices, largest drift {max(ck_drift):.3e}, "
          f"tolerance {tolerance:.3e}, smallest margin {out['margin'].min():.3e}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
