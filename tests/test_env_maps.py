"""CPU tests of the shared environment map generator (tests/support/env_maps.py): with default knobs it draws exactly
the maps of the generator tests/test_gpu_env.py used before it moved (kept verbatim below as the pin), and its knobs
reach the limits the environment kernels accept."""
import importlib

import numpy as np
import pytest

from support import env_maps  # noqa: E402
from trajtrack_mpcndqn_rlboost_amd import rl_env, rl_geometry as rg


# tests/test_gpu_env.py before the generator moved to tests/support/env_maps.py, unchanged
def _random_map_before_the_move(rng):
    """A random hall with random convex obstacles on general key-frame animations (1..4 key frames, linear or cosine
    easing, time offsets) -- exercises what the two fixture scenes do not: n_kf_max = 4, linear interpolation, offsets,
    different obstacle / edge / path-node counts per environment in one batch."""
    import math
    rg = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_geometry")
    W, H = rng.uniform(12, 30), rng.uniform(10, 25)
    boundary = [(0, 0), (W, 0), (W, H), (0, H)]
    if rng.random() < 0.5:                      # notch: a reflex corner in the boundary
        boundary = [(0, 0), (W, 0), (W, H * 0.6), (W * 0.7, H * 0.6), (W * 0.7, H), (0, H)]
    obstacles = []
    for _ in range(rng.integers(0, 7)):
        n = rng.integers(3, 7)
        ang = np.sort(rng.uniform(0, 2 * math.pi, n))
        if np.min(np.diff(np.concatenate([ang, [ang[0] + 2 * math.pi]]))) < 0.4:
            continue
        rad = rng.uniform(0.5, 2.0)
        nodes = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
        if rg.signed_area(nodes) < 0.3:
            continue
        nk = int(rng.integers(1, 5))
        frames = [(rng.uniform(1, W - 1), rng.uniform(1, H - 1), rng.uniform(-3, 3)) for _ in range(nk)]
        steps = [0.0] + [float(rng.uniform(0.5, 6.0)) for _ in range(nk)]
        obstacles.append(dict(padded_nodes=rg.buffer_polygon(nodes, 0.5), time_steps=steps, keyframes=frames,
                              interp="cosine" if rng.random() < 0.5 else "linear", offset=float(rng.uniform(0, 5))))
    npath = int(rng.integers(2, 9))
    path = np.stack([np.sort(rng.uniform(0.5, W - 0.5, npath)), rng.uniform(0.5, H * 0.55, npath)], axis=1)
    return dict(start=np.array([path[0, 0], path[0, 1], 0.0, 0.0, 0.0]), goal=np.asarray(path[-1], dtype=np.float32).astype(float),
                path=path, boundary_padded=rg.buffer_polygon(boundary, -0.5), obstacles=obstacles)


@pytest.mark.parametrize("seed,count", [(99, 96), (0, 40), (12345, 40)])
def test_default_knobs_draw_the_same_maps_as_before_the_move(seed, count):
    """Same records byte for byte, same batch maxima, and the generator left in the same state (the test that draws its
    actions from the same generator afterwards sees the same actions)."""
    r_old, r_new = np.random.default_rng(seed), np.random.default_rng(seed)
    old = [_random_map_before_the_move(r_old) for _ in range(count)]
    new = [env_maps.random_map(r_new) for _ in range(count)]
    rec_old, max_old = rl_env.pack_records(old)
    rec_new, max_new = rl_env.pack_records(new)
    assert max_old == max_new
    assert rec_old.shape == rec_new.shape and rec_old.tobytes() == rec_new.tobytes()
    for a, b in zip(old, new):
        assert [o["interp"] for o in a["obstacles"]] == [o["interp"] for o in b["obstacles"]]
    assert r_old.bit_generator.state == r_new.bit_generator.state


def _is_convex(ring):
    d = np.roll(ring, -1, axis=0) - ring
    cross = d[:, 0] * np.roll(d[:, 1], -1) - d[:, 1] * np.roll(d[:, 0], -1)
    return bool((cross >= -1e-12).all() or (cross <= 1e-12).all())


def test_knobs_reach_the_kernel_limits():
    rng = np.random.default_rng(7)
    m31 = env_maps.random_map(rng, n_obst=31, n_kf=(4, 5), interp="linear", concave=0.5)
    assert len(m31["obstacles"]) == 31
    assert all(len(o["keyframes"]) == 4 and len(o["time_steps"]) == 5 and o["interp"] == "linear" for o in m31["obstacles"])
    assert len({o["offset"] for o in m31["obstacles"]}) == 31
    assert any(not _is_convex(o["padded_nodes"]) for o in m31["obstacles"])
    for o in m31["obstacles"]:
        assert rg.signed_area(o["padded_nodes"]) > 0 and rg.ring_is_simple(o["padded_nodes"])
    m0 = env_maps.random_map(rng, n_obst=0, interp="cosine")
    assert m0["obstacles"] == []
    big = env_maps.random_map(rng, n_obst=3, boundary_vertices=300, n_edge=1017)
    assert env_maps.n_edges(big) == 1017 and len(big["boundary_padded"]) > 300
    ring = np.asarray(big["boundary_padded"])
    assert rg.signed_area(ring) > 0 and not _is_convex(ring)
    rec, maxima = rl_env.pack_records([m31, m0, big])
    assert maxima == dict(n_path_max=maxima["n_path_max"], n_obst_max=31, n_kf_max=4, n_edge_max=1017)
    assert rec[:, 1].tolist() == [31.0, 0.0, 3.0] and rec[2, 2] == 1017.0
    with pytest.raises(ValueError, match="outline edges"):
        env_maps.random_map(np.random.default_rng(1), n_obst=31, n_edge=40)
