"""The shape of ``DqnLearner.state_dict()``: every nested key in order, with the Python type of numbers and lists and the
dtype, shape and device type of tensors (the generator state is a uint8 tensor) -- no tensor values.  Shared by
``tests/golden/make_dqn_checkpoint_schema.py``, which records it, and ``tests/test_dqn_checkpoint_schema.py``, which compares.
It uses the learner's public arguments only, so it runs unchanged on any revision.

Every leg is the smallest run in which every branch of the checkpoint is populated: 8 environments whose episodes end within
10 steps, a ring of 64 rows that 12 calls wrap, batch 8, learning from 16 steps on, 2 gradient steps (Adam state exists) every
4 calls.  The image legs use 37 x 39 pixels: odd, unequal, and just above the 36 below which ``dqn.NatureCNN``'s three
convolutions have no output."""
import importlib
import json
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "dqn_checkpoint_schema.json")
GOLDEN = os.path.dirname(FIXTURE)
ENVS, CALLS, IMAGE_H, IMAGE_W = 8, 12, 37, 39
LEARNER = dict(buffer_size=64, learning_starts=16, batch_size=8, train_freq=4, gradient_steps=2, target_update_interval=32, seed=3)
# leg -> (environment, learner arguments); the first runs without a GPU
LEGS = {
    "ray_uniform_cpu": ("counting", {}),
    "ray_uniform": ("rays", {}),
    "ray_per": ("rays", dict(per=True)),
    "image_uniform": ("images", {}),
    "image_per": ("images", dict(per=True)),
    "ray_fused": ("rays", dict(fused=True)),
    "ray_fused_per": ("rays", dict(fused=True, per=True)),
    "ray_graph": ("rays", dict(use_graph=True)),
}
CPU_LEGS = tuple(leg for leg, (kind, _) in LEGS.items() if kind == "counting")
GPU_LEGS = tuple(leg for leg in LEGS if leg not in CPU_LEGS)


def _maps(rl_env):
    fx = np.load(os.path.join(GOLDEN, "env_rays_traces.npz"))
    specs = json.loads(bytes(fx["specs_json"]).decode())
    maps = [rl_env.make_map(sp["boundary"], sp["static"], sp["dynamic"], sp["start"], sp["goal"], sp["path"]) for sp in specs.values()]
    return [maps[i % 2] for i in range(ENVS)]


def make_env(kind):
    if kind == "counting":
        from test_dqn_learner import CountingEnv
        return CountingEnv(B=ENVS)
    rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
    if kind == "rays":
        return rl_env.BatchedRaysEnv(_maps(rl_env), max_episode_steps=10)
    return rl_env.BatchedImgsEnv(_maps(rl_env), max_episode_steps=10, image_height=IMAGE_H, image_width=IMAGE_W)


def checkpoint(leg):
    """``state_dict()`` of the leg's learner after ``CALLS`` environment calls."""
    dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
    kind, kw = LEGS[leg]
    torch.manual_seed(0)
    learner = dqn_train.DqnLearner(make_env(kind), **LEARNER, **kw)
    learner.learn(total_timesteps=ENVS * CALLS)
    assert learner.buffer.size == LEARNER["buffer_size"] and learner.buffer.pos == ENVS * CALLS % LEARNER["buffer_size"]
    assert learner.trainer.num_updates == 6 and learner.trainer.num_target_syncs == 3 and len(learner.episode_returns) > 0
    return learner.state_dict()


def walk(node, path=""):
    """[[path, description], ...] in the order the checkpoint holds its entries."""
    if isinstance(node, dict):
        out = [[path, f"dict of {len(node)}"]]
        for k, v in node.items():
            out += walk(v, f"{path}/{type(k).__name__}:{k}")
        return out
    if isinstance(node, torch.Tensor):
        return [[path, f"tensor {str(node.dtype).replace('torch.', '')} {list(node.shape)} {node.device.type}"]]
    if isinstance(node, (list, tuple)):
        if any(isinstance(v, (dict, list, tuple, torch.Tensor)) for v in node):
            out = [[path, f"{type(node).__name__} of {len(node)}"]]
            for i, v in enumerate(node):
                out += walk(v, f"{path}/{i}")
            return out
        return [[path, f"{type(node).__name__} of {'|'.join(sorted({type(v).__name__ for v in node}))}"]]    # a run decides its length
    return [[path, type(node).__name__]]


def schema(leg):
    return walk(checkpoint(leg))


def load(path=FIXTURE):
    with open(path) as fh:
        return json.load(fh)


def differences(got, want):
    """The entries in which two walks differ, first one first: a renamed, missing, extra or reordered key shifts the walk."""
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    if len(got) != len(want):
        n = min(len(got), len(want))
        bad.append((n, got[n] if len(got) > n else None, want[n] if len(want) > n else None))
    return bad
