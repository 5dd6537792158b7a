"""TEST INFRASTRUCTURE -- CPU twin of the bookkeeping rule of include/mpcgpu_eval.h, and of nothing else.

The environment and the policy are replaced by a SCRIPT: ``script[b][i]`` is what row b's i-th step of the evaluation gives,
``(reward, terminated, truncated, flags)`` -- the step a row makes depends on the row's own step count alone, as it does in the
kernel, where the state and the serial ``serial0 + steps_done[b]`` carry it.  :func:`launch` is one launch of up to S trips per
row on the progress vectors and the three [B][E] outputs, all numpy arrays updated in place."""
from __future__ import annotations

import numpy as np

from . import collect_numpy as cn

PROGRESS = (("episodes_done", np.int32), ("steps_done", np.int64), ("ep_return", np.float64), ("ep_length", np.int32))
OUTPUTS = (("returns", np.float64), ("lengths", np.int32), ("outcome", np.uint8))


def new_progress(B: int):
    return {name: np.zeros(B, dtype) for name, dtype in PROGRESS}


def new_out(B: int, E: int, fill=0):
    return {name: np.full((B, E), fill, dtype) for name, dtype in OUTPUTS}


def launches_that_suffice(E: int, max_episode_steps: int, S: int) -> int:
    return -(-E * max_episode_steps // S)


def launch(script, progress, out, E: int, S: int, serial0: int = 0, serials=None) -> int:
    """One launch.  ``serials[b]``, when given, collects the serial of every trip row b makes.  Returns the trips made in all."""
    trips = 0
    for b in range(len(script)):
        if progress["episodes_done"][b] >= E:
            continue                                                          # parked: nothing of the row is read or written
        done, made = int(progress["episodes_done"][b]), int(progress["steps_done"][b])
        ret, length = np.float64(progress["ep_return"][b]), int(progress["ep_length"][b])
        for _ in range(S):
            if serials is not None:
                serials[b].append((serial0 + made) % 2 ** 64)
            reward, terminated, truncated, flags = script[b][made]
            ret = np.float64(ret + np.float64(reward))                        # one double addition
            length += 1
            made += 1
            trips += 1
            if terminated or truncated:
                out["returns"][b, done], out["lengths"][b, done] = ret, length
                out["outcome"][b, done] = (int(flags) & 7) | (8 if truncated else 0)
                ret, length, done = np.float64(0.0), 0, done + 1
            if done >= E:
                break
        progress["episodes_done"][b], progress["steps_done"][b] = done, made
        progress["ep_return"][b], progress["ep_length"][b] = ret, length
    return trips


def explored(seed: int, serial0: int, steps, b: int, eps: float) -> bool:
    """Whether row b explores in one of its steps ``steps`` (its own step counts) of the stream ``(seed, serial0 + step)``."""
    return any(cn.uniform_of(cn.draw_bits(seed, (serial0 + s) % 2 ** 64, b)[0]) < eps for s in steps)
