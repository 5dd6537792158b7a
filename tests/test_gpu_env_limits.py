"""GPU tests of the environment kernels at the limits they accept, on seeded random maps (tests/support/env_maps.py):
31 and 0 obstacles, 1..4 key frames with linear and cosine easing, concave outlines, edge counts up to the LDS bound of
the image kernel, image sides 8..96 on both store paths, and vertices at the +-2^20 px clamp.

Images must equal the numpy restatement (tests/support/image_obs_numpy.py) exactly, with the exemption of
tests/test_gpu_env_imgs.py (a vertex within 1e-9 px of where its pixel changes; fewer than 1 % of the images).  The
non-image outputs of the image variant must equal BatchedRaysEnv bit for bit; the ray kernel itself is compared with the
oracle at the tolerances of tests/test_gpu_env.py."""
import importlib
import math
import time

import numpy as np
import pytest
import torch

from oracle import rl_env_numpy as orc
from support import env_maps  # noqa: E402
from support import image_obs_numpy as im  # noqa: E402

pytestmark = pytest.mark.gpu
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
LEVELS = {0, 64, 128, 191, 255}
# the largest n_edge_max the image kernel accepts: 2 * E * sizeof(EdgePix) (48 B per edge) + sizeof(Shared) (16 712 B)
# must fit 64 KiB of LDS
E_LIMIT = 1017


def image_env(maps, W=54, H=54, scale_x=1 / 18, scale_y=1 / 18, cx=0.5, cy=0.3, angle=0.0, **kw):
    env = rl_env.BatchedImgsEnv(maps, image_width=W, image_height=H, image_scale_x=scale_x, image_scale_y=scale_y,
                                image_center_x=cx, image_center_y=cy, image_angle=angle, **kw)
    ip = im.ImageParams(W, H, scale_x, scale_y, 2, cx, cy, angle)
    dfield = im.distance_field(W, H, scale_x, scale_y, cx, cy)
    assert np.array_equal(env.distance_field.cpu().numpy(), dfield)
    return env, ip, dfield


class Tally:
    """Compares images with the restatement and counts what was compared."""

    def __init__(self):
        self.total = self.ambiguous = self.compared = 0
        self.counts = {}

    def check(self, got, spec, pose, c0, c1, ip, dfield, what, tags=()):
        want, amb = im.render_pair(spec, pose, c0, c1, ip, dfield)
        self.total += 1
        if amb:
            self.ambiguous += 1
            return False
        diff = np.argwhere(got != want)
        assert diff.size == 0, (what, diff[:5].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
        assert set(np.unique(got[:2]).tolist()) <= LEVELS
        self.compared += 1
        for t in tags:
            self.counts[t] = self.counts.get(t, 0) + 1
        return True

    def finish(self, label):
        print(f"[limits] {label}: {self.compared} images compared exactly, {self.ambiguous} of {self.total} ambiguous; "
              + ", ".join(f"{k}: {v}" for k, v in sorted(self.counts.items())))
        assert self.ambiguous < 0.01 * self.total


def map_tags(m):
    obs = m["obstacles"]
    tags = [f"M={len(obs)}"]
    if len(obs) == 31 and all(len(o["keyframes"]) == 4 and o["interp"] == "linear" for o in obs):
        tags.append("M=31 K=4 linear")
    if any(not _convex(o["padded_nodes"]) for o in obs):
        tags.append("concave")
    tags += sorted({f"K={len(o['keyframes'])} {o['interp']}" for o in obs})
    return tags


def _convex(ring):
    d = np.roll(ring, -1, axis=0) - ring
    cross = d[:, 0] * np.roll(d[:, 1], -1) - d[:, 1] * np.roll(d[:, 0], -1)
    return bool((cross >= -1e-12).all() or (cross <= 1e-12).all())


def mixed_maps(seed):
    """One batch across the limits: M = 31 and 0, K = 1..4, linear and cosine, concave outlines, wavy boundaries,
    different edge counts per environment."""
    rng = np.random.default_rng(seed)
    knobs = [dict(n_obst=31, n_kf=(4, 5), interp="linear", concave=0.2, n_vert=(3, 5)),
             dict(n_obst=31, n_kf=(1, 5), concave=0.2, n_vert=(3, 5)),
             dict(n_obst=31, n_kf=(3, 4), interp="cosine", n_vert=(3, 4)),
             dict(n_obst=0), dict(n_obst=0, boundary_vertices=60),
             dict(), dict(), dict(),
             dict(n_obst=(10, 20), n_kf=(2, 4), concave=0.5),
             dict(n_obst=31, n_kf=(4, 5), interp="linear", n_vert=(3, 4)),
             dict(n_obst=8, boundary_vertices=40, interp="linear"),
             dict(n_obst=(1, 4), n_kf=(1, 2), interp="cosine", concave=1.0),
             dict(n_obst=(3, 8), offset=(0.0, 40.0), concave=0.3),
             dict(n_obst=1, n_kf=(4, 5), interp="linear"),
             dict(n_obst=0, boundary_vertices=25, n_edge=300),
             dict(n_obst=31, concave=0.1, n_vert=(3, 5), boundary_vertices=30)]
    maps = [env_maps.random_map(rng, **k) for k in knobs]
    assert max(env_maps.n_edges(m) for m in maps) <= E_LIMIT
    return maps


def test_mixed_limit_batch_with_autoreset_matches_the_restatement_and_the_ray_variant():
    t0 = time.time()
    maps = mixed_maps(2024)
    B, LIMIT = len(maps), 11
    assert len({env_maps.n_edges(m) for m in maps}) >= 10 and {0, 31} <= {len(m["obstacles"]) for m in maps}
    env, ip, dfield = image_env(maps, max_episode_steps=LIMIT, time_step=0.15)
    ref = rl_env.BatchedRaysEnv(maps, max_episode_steps=LIMIT, time_step=0.15)
    assert env.params.n_obst_max == 31 and env.params.n_kf_max == 4
    tags = [map_tags(m) for m in maps]
    tally = Tally()
    hists = [im.ImageHistory() for _ in range(B)]
    obs, robs = env.reset(), ref.reset()
    st = env.state.cpu().numpy()
    for b in range(B):
        tally.check(obs["external"][b].cpu().numpy(), maps[b], st[b, :3], *hists[b].push(0.0), ip, dfield, ("reset", b),
                    tags[b])
    rng = np.random.default_rng(7)
    n_obs = [1] * B
    ended = {"terminated": 0, "truncated": 0}
    n_terminal_imgs = n_late = 0
    for t in range(28):
        acts = rng.integers(0, 9, B)
        acts[3] = acts[4] = 7                       # brake / reverse slowly in the empty halls: ends by the time limit
        acts[[0, 1, 5, 6, 8, 12]] = 1 if t % 5 else 0   # mostly accelerating straight on: ends by a collision
        a = torch.from_numpy(acts)
        obs, rew, term, trunc, info = env.step(a, auto_reset=True)
        robs, rrew, rterm, rtrunc, rinfo = ref.step(a, auto_reset=True)
        assert torch.equal(rew, rrew) and torch.equal(term, rterm) and torch.equal(trunc, rtrunc)
        assert torch.equal(info["success"], rinfo["success"])
        assert torch.equal(obs["internal"], robs["internal"])
        assert torch.equal(info["terminal_observation"]["internal"], rinfo["terminal_observation"]["internal"])
        assert torch.equal(env.state, ref.state)
        done, term_np = (term | trunc).cpu().numpy(), term.cpu().numpy()
        st, ist = env.state.cpu().numpy(), env.img_state.cpu().numpy()
        img, timg = obs["external"].cpu().numpy(), info["terminal_observation"]["external"].cpu().numpy()
        for b in range(B):
            if done[b]:
                pre = ist[b, 8:12]                  # pose and clock the step observed before the in-kernel reset
                c0, c1 = hists[b].push(pre[3])
                n_terminal_imgs += tally.check(timg[b], maps[b], pre[:3], c0, c1, ip, dfield, ("terminal", t, b),
                                               tags[b] + ["terminal"])
                hists[b].reset()
                ended["terminated" if term_np[b] else "truncated"] += 1
                assert st[b, 5] == 0.0 and np.array_equal(st[b, :5], maps[b]["start"])
            c0, c1 = hists[b].push(st[b, 5])
            late = c1 != 0.0                        # channel 1 shows an observation after the reset
            n_late += tally.check(img[b], maps[b], st[b, :3], c0, c1, ip, dfield, ("step", t, b),
                                  tags[b] + (["channel 1 after the reset"] if late else [])) and late
            if not done[b]:
                assert np.array_equal(timg[b], img[b])
            n_obs[b] = 1 if done[b] else n_obs[b] + 1
        assert ist[:, 0].tolist() == [float(n) for n in n_obs]
    tally.finish(f"mixed batch B = {B}, {time.time() - t0:.1f} s")
    assert ended["terminated"] >= 5 and ended["truncated"] >= 5, ended
    assert n_terminal_imgs >= 5 and n_late >= 20
    assert tally.counts.get("M=31 K=4 linear", 0) >= 20 and tally.counts.get("M=0", 0) >= 20
    assert tally.counts.get("concave", 0) >= 20 and all(tally.counts.get(f"K={k} linear", 0) > 0 for k in (1, 2, 3, 4))


SIZES = [(8, 8), (9, 11), (32, 33), (33, 32), (64, 65), (65, 64), (96, 96), (95, 9)]
assert any((W * H) % 4 for W, H in SIZES) and any((W * H) % 4 == 0 for W, H in SIZES)


@pytest.mark.parametrize("W,H", SIZES)
def test_image_sizes_word_edges_and_both_store_paths(W, H):
    """2W = 64 / 66 / 128 / 130 put the right image edge on, or 2 bits past, a 64-bit word of the bit planes; an odd
    H * W makes the kernel write bytes instead of 32-bit words."""
    t0 = time.time()
    byte_path = (W * H) % 4 != 0
    rng = np.random.default_rng(W * 1000 + H)
    maps = [env_maps.random_map(rng, **k) for k in
            [dict(), dict(n_obst=31, n_vert=(3, 4), n_kf=(4, 5), interp="linear"), dict(n_obst=0, boundary_vertices=30),
             dict(concave=0.5, n_obst=(4, 9))] * 4]
    B = len(maps)
    cx, cy, angle = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(-3, 3)
    env, ip, dfield = image_env(maps, W, H, 1 / 22, 1 / 19, cx, cy, angle)
    assert env.obs_image.shape == (B, 3, H, W)
    hists = [im.ImageHistory() for _ in range(B)]
    env.reset()
    for h in hists:
        h.push(0.0)
    tally = Tally()
    for rep in range(4):
        states = np.zeros((B, 5))
        for b, m in enumerate(maps):
            ring = np.asarray(m["boundary_padded"])
            states[b] = [rng.uniform(ring[:, 0].min() - 2, ring[:, 0].max() + 2),
                         rng.uniform(ring[:, 1].min() - 2, ring[:, 1].max() + 2), rng.uniform(-4, 4), 0.0, 0.0]
        clock = rng.uniform(0.0, 40.0, B)
        env.set_agent_state(states)
        env.state[:, 5] = torch.from_numpy(clock).to(env.device)
        img = env.observe()["external"].cpu().numpy()
        st = env.state.cpu().numpy()
        for b in range(B):
            c0, c1 = hists[b].push(clock[b])
            shown = img[b, :2]
            tally.check(img[b], maps[b], st[b, :3], c0, c1, ip, dfield, (rep, b),
                        ["byte path" if byte_path else "word path"]
                        + (["both levels in the last column"] if {0, 255} <= set(shown[:, :, -1].ravel().tolist()) else []))
    tally.finish(f"{W}x{H} ({'byte' if byte_path else 'word'} path, 2W = {2 * W}), {time.time() - t0:.1f} s")
    assert tally.compared >= 3 * B
    assert tally.counts.get("both levels in the last column", 0) >= 2   # the right edge is not blank


def _clamped(spec, pose, c0, c1, ip):
    """Whether a vertex of the image pair is clamped to +-2^20 px."""
    rings = [np.asarray(spec["boundary_padded"], dtype=np.float64)]
    rings += [im.obstacle_world(ob, c) for c in (c0, c1) for ob in spec["obstacles"]]
    return any((np.abs(im.to_pixels(r, pose, ip)[0]) >= 2 ** 20).any() for r in rings)


@pytest.mark.parametrize("sx,sy", [(2000.0, 2500.0), (2e6, 2e6)])
def test_vertices_at_the_pixel_clamp(sx, sy):
    """At 216 000 px per metre every vertex farther than ~4.9 m from the robot is clamped to +-2^20 px; at 2.16e8 px per
    metre the unclamped coordinates reach 6e9 px, past int32 and past what the 16.16 fill could hold in 64 bits.  Robots
    placed within a few pixels of an edge see that edge cross the image, and near-axis-aligned headings make the fill
    slopes reach 2^37 in 16.16 (2^21 px across one row)."""
    t0 = time.time()
    rng = np.random.default_rng(31)
    maps = [env_maps.random_map(rng, **k) for k in
            [dict(), dict(n_obst=31, n_vert=(3, 4)), dict(n_obst=0, boundary_vertices=30), dict(concave=1.0, n_obst=6)] * 6]
    B = len(maps)
    W = H = 54
    env, ip, dfield = image_env(maps, W, H, sx, sy, 0.5, 0.4, 0.3)
    env.reset()
    hists = [im.ImageHistory() for _ in range(B)]
    for h in hists:
        h.push(0.0)
    tally = Tally()
    n_clamped_both = 0
    for rep in range(3):
        clock = rng.uniform(0.0, 30.0, B)
        states = np.zeros((B, 5))
        for b, m in enumerate(maps):
            obs = m["obstacles"]
            if obs and rng.random() < 0.5:
                ring = im.obstacle_world(obs[int(rng.integers(len(obs)))], clock[b])
            else:
                ring = np.asarray(m["boundary_padded"])
            k = int(rng.integers(len(ring)))
            p0, p1 = ring[k], ring[(k + 1) % len(ring)]
            d = p1 - p0
            nrm = np.array([-d[1], d[0]]) / np.hypot(*d)
            pt = p0 + rng.uniform(0.1, 0.9) * d + nrm * rng.uniform(-3, 3) / (2 * W * sx)
            phi = math.atan2(d[1], d[0]) + ip.angle
            jitter = [0.0, rng.uniform(-1e-6, 1e-6), rng.uniform(-1e-3, 1e-3), rng.uniform(-4, 4)][int(rng.integers(4))]
            states[b] = [pt[0], pt[1], phi + int(rng.integers(4)) * math.pi / 2 + jitter, 0.0, 0.0]
        env.set_agent_state(states)
        env.state[:, 5] = torch.from_numpy(clock).to(env.device)
        img = env.observe()["external"].cpu().numpy()
        st = env.state.cpu().numpy()
        for b in range(B):
            c0, c1 = hists[b].push(clock[b])
            clamped = _clamped(maps[b], st[b, :3], c0, c1, ip)
            levels = set(img[b, :2].ravel().tolist())
            both = clamped and {0, 255} <= levels
            n_clamped_both += tally.check(img[b], maps[b], st[b, :3], c0, c1, ip, dfield, (rep, b),
                                          ["clamped vertex"] * clamped + ["clamped vertex, 0 and 255"] * both) and both
    tally.finish(f"clamp, {sx:g} / {sy:g} px per image side, {time.time() - t0:.1f} s")
    # otherwise the test proves nothing: compared images that show both levels and have a clamped vertex
    assert n_clamped_both >= 10, n_clamped_both


def test_edge_count_at_the_lds_bound():
    """n_edge_max = 1017 fits the image kernel's LDS and draws exact images; 1018 is refused before anything runs."""
    t0 = time.time()
    rng = np.random.default_rng(1017)
    maps = [env_maps.random_map(rng, n_obst=5, boundary_vertices=120, n_edge=E_LIMIT),
            env_maps.random_map(rng, n_obst=31, n_vert=(3, 5), n_kf=(4, 5), interp="linear", n_edge=E_LIMIT),
            env_maps.random_map(rng), env_maps.random_map(rng, n_obst=0)]
    B = len(maps)
    env, ip, dfield = image_env(maps, 48, 40, 1 / 16, 1 / 16, 0.5, 0.3)
    ref = rl_env.BatchedRaysEnv(maps)
    assert env.params.n_edge_max == E_LIMIT and [env_maps.n_edges(m) for m in maps][:2] == [E_LIMIT, E_LIMIT]
    tags = [["E at the bound"] if env_maps.n_edges(m) == E_LIMIT else [] for m in maps]
    tally = Tally()
    hists = [im.ImageHistory() for _ in range(B)]
    obs, _ = env.reset(), ref.reset()
    st = env.state.cpu().numpy()
    for b in range(B):
        tally.check(obs["external"][b].cpu().numpy(), maps[b], st[b, :3], *hists[b].push(0.0), ip, dfield, b, tags[b])
    for t in range(8):
        a = torch.from_numpy(rng.integers(0, 9, B))
        obs, rew, term, trunc, _ = env.step(a)
        robs, rrew, rterm, rtrunc, _ = ref.step(a)
        assert torch.equal(rew, rrew) and torch.equal(term, rterm) and torch.equal(obs["internal"], robs["internal"])
        assert torch.equal(env.state, ref.state)
        st = env.state.cpu().numpy()
        img = obs["external"].cpu().numpy()
        for b in range(B):
            tally.check(img[b], maps[b], st[b, :3], *hists[b].push(st[b, 5]), ip, dfield, (t, b), tags[b])
    tally.finish(f"E = {E_LIMIT}, {time.time() - t0:.1f} s")
    assert tally.counts.get("E at the bound", 0) >= 12

    # one edge more: refused by the host check, before the step kernel is enqueued
    over = [env_maps.random_map(np.random.default_rng(1018), n_obst=3, boundary_vertices=80, n_edge=E_LIMIT + 1)] + maps[2:]
    bad, _, _ = image_env(over, 48, 40, 1 / 16, 1 / 16, 0.5, 0.3)
    assert bad.params.n_edge_max == E_LIMIT + 1
    starts = np.stack([np.asarray(m["start"]) for m in over])
    starts[:, 3] = 1.0                              # moving: a step that ran would change x, y and the clock
    bad.set_agent_state(starts)
    bad.state[:, 5] = 2.5
    bad.img_state.copy_(torch.arange(bad.img_state.numel(), dtype=torch.float64).reshape(bad.img_state.shape))
    bad.obs_image.fill_(77)
    bad.obs_internal.fill_(-3.0)
    torch.cuda.synchronize()
    before = bad.state_dict()
    acts = torch.full((len(over),), 1)
    for call in (bad.observe, lambda: bad.step(acts), lambda: bad.step(acts, auto_reset=True)):
        with pytest.raises(rl_env.MpcGpuError, match="too many outline edges"):
            call()
        torch.cuda.synchronize()
        after = bad.state_dict()
        for k in ("state", "img_state", "obs_image", "obs_internal", "reward", "terminated", "truncated"):
            assert after[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), k


def test_ray_kernel_at_31_obstacles_and_a_thousand_edges_matches_the_oracle():
    """env_step_kernel (the first kernel of every image step too) against OracleRaysEnv at M = 31 and E ~ 1000."""
    t0 = time.time()
    rng = np.random.default_rng(31000)
    maps = [env_maps.random_map(rng, n_obst=31, n_kf=(4, 5), interp="linear", concave=0.2, n_vert=(3, 5)),
            env_maps.random_map(rng, n_obst=31, concave=0.2, n_vert=(3, 5)),
            env_maps.random_map(rng, n_obst=31, n_vert=(3, 4), n_kf=(1, 3), interp="cosine"),
            env_maps.random_map(rng, n_obst=31, n_vert=(3, 4), n_edge=1000),
            env_maps.random_map(rng, n_obst=4, boundary_vertices=100, n_edge=1000),
            env_maps.random_map(rng, n_obst=0, boundary_vertices=100, n_edge=990),
            env_maps.random_map(rng, n_obst=12, concave=0.5, boundary_vertices=60, n_edge=1017),
            env_maps.random_map(rng), env_maps.random_map(rng, n_obst=0)]
    B = len(maps)
    env = rl_env.BatchedRaysEnv(maps, time_step=0.15)
    assert env.params.n_obst_max == 31 and env.params.n_edge_max == 1017
    oracles = [orc.OracleRaysEnv(m, time_step=0.15) for m in maps]
    env.reset()
    n_collided = 0
    for k in range(10):
        acts = rng.integers(0, 9, B)
        if k % 4 == 3:                              # teleport everybody, anywhere in (or slightly outside) the hall
            st = np.zeros((B, 5))
            for b, m in enumerate(maps):
                ring = np.asarray(m["boundary_padded"])
                st[b] = [rng.uniform(ring[:, 0].min() - 0.3, ring[:, 0].max() + 0.3),
                         rng.uniform(ring[:, 1].min() - 0.3, ring[:, 1].max() + 0.3), rng.uniform(-4, 4),
                         rng.uniform(-0.5, 1.5), rng.uniform(-0.5, 0.5)]
                oracles[b].state[:] = st[b]
            env.set_agent_state(st)
        obs, rew, term, _, _ = env.step(torch.from_numpy(acts))
        oi, oe = obs["internal"].cpu().numpy(), obs["external"].cpu().numpy()
        st, fl = env.agent_state.cpu().numpy(), env.flags.cpu().numpy()
        for b, o in enumerate(oracles):
            ob, r, done, _ = o.step(int(acts[b]))
            assert np.abs(st[b] - o.state).max() <= 1e-12, (k, b)
            assert np.array_equal(fl[b], [o.collided_obstacle, o.collided_boundary, o.reached_goal]), (k, b)
            assert np.abs(oi[b] - ob["internal"]).max() <= 1e-6, (k, b)
            assert np.abs(oe[b] - ob["external"]).max() <= 2e-6, (k, b, oe[b], ob["external"])
            assert abs(float(rew[b]) - r) <= 1e-9 and bool(term[b]) == done
            n_collided += int(o.collided)
    print(f"[limits] ray kernel: {B} maps x 10 steps, M = {[len(m['obstacles']) for m in maps]}, "
          f"E = {[env_maps.n_edges(m) for m in maps]}, {n_collided} collided, {time.time() - t0:.1f} s")
    assert n_collided > 0
