"""GPU tests of the image-observation environment (``rl_env.BatchedImgsEnv``, csrc/envimg.hip) against the numpy
restatement of tests/support/image_obs_numpy.py.  Images must equal the restatement exactly: everything after the
truncation to integer pixels is integer arithmetic.  The restatement is driven by the kernel's own robot pose and clock
(float64, bit-identical to the ray variant's), so what is compared is the image rule alone.  Only images with a vertex
within 1e-9 px of an integer before truncation are exempt (there a last-ulp difference of a libm cos / sin may move a
vertex across the boundary; a coordinate clamped to +-2^20 px counts by its distance to the clamp); the random-state test
reports how many and bounds them."""
import ctypes as C
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from support import image_obs_numpy as im  # noqa: E402

pytestmark = pytest.mark.gpu
rl_env = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.rl_env")
dqn_train = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.dqn_train")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "env_rays_traces.npz")
LEVELS = {0, 64, 128, 191, 255}


def load():
    fx = np.load(GOLD)
    specs = json.loads(bytes(fx["specs_json"]).decode())
    maps = {name: rl_env.make_map(sp["boundary"], sp["static"], sp["dynamic"], sp["start"], sp["goal"], sp["path"])
            for name, sp in specs.items()}
    return fx, maps


def expect(spec, state_row, c0, c1, ip, dfield):
    return im.render_pair(spec, state_row[:3], c0, c1, ip, dfield)


def test_traces_images_exact_and_non_image_outputs_equal_the_ray_variant():
    """Both fixture maps in one batch, driven by their recorded actions: every image equals the restatement, and internal
    observation, reward, flags and state[0:8] equal BatchedRaysEnv bit for bit."""
    fx, maps = load()
    keys = ["scene1_r0", "lhall_r0"]
    specs = [maps[k.split("_")[0]] for k in keys]
    ts = float(fx[keys[0] + "_ts"])
    env = rl_env.BatchedImgsEnv(specs, time_step=ts)
    ref = rl_env.BatchedRaysEnv(specs, time_step=ts)
    ip = im.ImageParams()
    dfield = im.distance_field(54, 54, 1 / 18, 1 / 18, 0.5, 0.3)
    hists = [im.ImageHistory() for _ in keys]
    obs, robs = env.reset(), ref.reset()
    steps = min(len(fx[k + "_actions"]) for k in keys)
    n_checked = 0
    for t in range(steps + 1):
        if t > 0:
            acts = torch.tensor([int(fx[k + "_actions"][t - 1]) for k in keys])
            obs, rew, term, trunc, info = env.step(acts)
            robs, rrew, rterm, rtrunc, rinfo = ref.step(acts)
            assert torch.equal(rew, rrew) and torch.equal(term, rterm) and torch.equal(trunc, rtrunc)
            assert torch.equal(info["success"], rinfo["success"])
        assert torch.equal(obs["internal"], robs["internal"])
        assert torch.equal(env.state[:, :8], ref.state[:, :8])
        img = obs["external"].cpu().numpy()
        st = env.state.cpu().numpy()
        assert img.dtype == np.uint8 and img.shape == (2, 3, 54, 54)
        for b in range(len(keys)):
            c0, c1 = hists[b].push(st[b, 5])
            want, _ = expect(specs[b], st[b], c0, c1, ip, dfield)
            diff = np.argwhere(img[b] != want)
            assert diff.size == 0, (keys[b], t, diff[:5].tolist())
            assert set(np.unique(img[b, :2]).tolist()) <= LEVELS
            n_checked += 1
    assert n_checked == 2 * (steps + 1)
    # the boundary and at least one obstacle are visible somewhere along the traces
    assert (img[:, 0] == 255).any() and (img[:, 0] == 0).any()


@pytest.mark.parametrize("W,H,cx,cy,angle,scale", [(54, 54, 0.5, 0.3, 0.0, 1 / 18), (32, 48, 0.2, 0.7, 1.1, 1 / 9),
                                                   (96, 96, 0.5, 0.5, -2.5, 1 / 30), (8, 17, 1.3, -0.4, 3.0, 1 / 5)])
def test_random_states_and_clocks(W, H, cx, cy, angle, scale):
    fx, maps = load()
    specs = [maps["scene1"], maps["lhall"]] * 48
    B = len(specs)
    env = rl_env.BatchedImgsEnv(specs, image_width=W, image_height=H, image_center_x=cx, image_center_y=cy,
                                image_angle=angle, image_scale_x=scale, image_scale_y=scale * 1.25)
    ip = im.ImageParams(W, H, scale, scale * 1.25, 2, cx, cy, angle)
    dfield = im.distance_field(W, H, scale, scale * 1.25, cx, cy)
    assert np.array_equal(env.distance_field.cpu().numpy(), dfield)
    rng = np.random.default_rng(W * 1000 + H)
    env.reset()
    total = ambiguous = 0
    clocks = []
    for rep in range(3):
        lo = np.array([-3.0, -3.0])
        hi = np.array([18.0, 14.0])   # beyond both boundaries: robots outside the map too
        xy = rng.uniform(lo, hi, (B, 2))
        states = np.column_stack([xy, rng.uniform(0, 2 * math.pi, B), rng.uniform(-0.5, 1.5, B), rng.uniform(-0.5, 0.5, B)])
        clock = rng.uniform(0.0, 30.0, B)
        env.set_agent_state(states)
        env.state[:, 5] = torch.from_numpy(clock).to(env.device)
        obs = env.observe()
        clocks.append(clock)
        img = obs["external"].cpu().numpy()
        st = env.state.cpu().numpy()
        for b in range(B):
            want, amb = expect(specs[b], st[b], clock[b], 0.0, ip, dfield)   # 4 observations < 6: oldest = the reset (clock 0)
            total += 1
            if amb:
                ambiguous += 1
                continue
            diff = np.argwhere(img[b] != want)
            assert diff.size == 0, (rep, b, st[b, :3].tolist(), clock[b], diff[:5].tolist())
        assert set(np.unique(img[:, :2]).tolist()) <= LEVELS
    print(f"[imgs] {W}x{H}: {ambiguous} of {total} images ambiguous (vertex within 1e-9 px of an integer)")
    assert ambiguous < 0.01 * total
    assert env.img_state[:, 0].cpu().tolist() == [4.0] * B   # the reset plus three observe-only calls


def test_autoreset_terminal_images_history_and_masked_reset():
    fx, maps = load()
    specs = [maps["scene1"], maps["lhall"]] * 4
    B = len(specs)
    env = rl_env.BatchedImgsEnv(specs, max_episode_steps=9)
    ip = im.ImageParams()
    dfield = im.distance_field(54, 54, 1 / 18, 1 / 18, 0.5, 0.3)
    hists = [im.ImageHistory() for _ in range(B)]
    obs = env.reset()
    st = env.state.cpu().numpy()
    for b in range(B):
        assert np.array_equal(obs["external"][b].cpu().numpy(), expect(specs[b], st[b], *hists[b].push(0.0), ip, dfield)[0])
    rng = np.random.default_rng(5)
    n_terminal = n_trunc = 0
    n_obs = [1.0] * B
    for t in range(40):
        acts = torch.from_numpy(rng.integers(0, 9, B))
        obs, rew, term, trunc, info = env.step(acts, auto_reset=True)
        done = (term | trunc).cpu().numpy()
        st, ist = env.state.cpu().numpy(), env.img_state.cpu().numpy()
        img, timg = obs["external"].cpu().numpy(), info["terminal_observation"]["external"].cpu().numpy()
        for b in range(B):
            if done[b]:
                pre = ist[b, 8:12]   # pose and clock the step observed before the in-kernel reset
                want, amb = expect(specs[b], pre, *hists[b].push(pre[3]), ip, dfield)
                assert amb or np.array_equal(timg[b], want), (t, b)
                hists[b].reset()
                n_terminal += int(term[b]); n_trunc += int(trunc[b])
                assert st[b, 5] == 0.0 and np.array_equal(st[b, :5], specs[b]["start"])
            want, amb = expect(specs[b], st[b], *hists[b].push(st[b, 5]), ip, dfield)
            assert amb or np.array_equal(img[b], want), (t, b)
            if not done[b]:
                assert np.array_equal(timg[b], img[b])
        for b in range(B):
            n_obs[b] = 1 if done[b] else n_obs[b] + 1
        assert ist[:, 0].tolist() == n_obs
    assert n_trunc > 0
    # masked reset: the other rows keep state, history and image bit for bit
    for _ in range(3):
        env.step(torch.from_numpy(rng.integers(0, 9, B)))
    mask = torch.tensor([i % 3 == 0 for i in range(B)], device=env.device)
    before = {k: v.clone() for k, v in env.state_dict().items()}
    obs = env.reset(mask)
    keep = ~mask
    for k in ("state", "img_state", "obs_internal", "obs_image", "reward", "terminated"):
        assert torch.equal(env.state_dict()[k][keep], before[k][keep]), k
    st = env.state.cpu().numpy()
    for b in np.flatnonzero(mask.cpu().numpy()):
        assert env.img_state[b, 0].item() == 1.0
        want, _ = expect(specs[b], st[b], 0.0, 0.0, ip, dfield)
        assert np.array_equal(obs["external"][b].cpu().numpy(), want)
    # observe-only pushes the history of every row
    n0 = env.img_state[:, 0].clone()
    env.observe()
    assert torch.equal(env.img_state[:, 0], n0 + 1)


def test_invalid_calls_fail_loudly():
    fx, maps = load()
    specs = [maps["lhall"]] * 2
    with pytest.raises(ValueError, match="down_sample"):
        rl_env.BatchedImgsEnv(specs, image_down_sample=3)
    with pytest.raises(ValueError, match="8..96"):
        rl_env.BatchedImgsEnv(specs, image_width=100)
    env = rl_env.BatchedImgsEnv(specs)
    env.reset()
    with pytest.raises(ValueError):
        env.step(torch.zeros(3, dtype=torch.int32))
    lib = env._lib
    stream = torch.cuda.current_stream(env.device).cuda_stream
    rc = lib.mpcgpu_env_step_imgs_dev(0, C.byref(env.params), C.byref(env.img_params), 2, env.records.data_ptr(),
                                      env.state.data_ptr(), None, env.distance_field.data_ptr(), None,
                                      env.obs_internal.data_ptr(), env.obs_image.data_ptr(), None, None, stream)
    assert rc < 0 and b"null" in lib.mpcgpu_env_last_error()
    acts = torch.zeros(2, dtype=torch.int32, device=env.device)
    rc = lib.mpcgpu_env_step_imgs_autoreset_dev(0, C.byref(env.params), C.byref(env.img_params), 2, env.records.data_ptr(),
                                                env.state.data_ptr(), env.img_state.data_ptr(), env.distance_field.data_ptr(),
                                                acts.data_ptr(), env.obs_internal.data_ptr(), env.obs_image.data_ptr(), None,
                                                None, None, None, None, 0, stream)
    assert rc < 0 and b"max_episode_steps" in lib.mpcgpu_env_last_error()
    bad = rl_env.image_params(down_sample=4)
    rc = lib.mpcgpu_env_step_imgs_dev(0, C.byref(env.params), C.byref(bad), 2, env.records.data_ptr(), env.state.data_ptr(),
                                      env.img_state.data_ptr(), env.distance_field.data_ptr(), None,
                                      env.obs_internal.data_ptr(), env.obs_image.data_ptr(), None, None, stream)
    assert rc < 0 and b"down_sample" in lib.mpcgpu_env_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="use_graph"):
        dqn_train.DqnLearner(env, buffer_size=64, use_graph=True)


def test_dqn_learner_on_the_image_environment_resumes_exactly(tmp_path):
    fx, maps = load()
    specs = [maps["scene1"], maps["lhall"]]
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False

    def make(seed):
        torch.manual_seed(0)
        env = rl_env.BatchedImgsEnv([specs[i % 2] for i in range(32)], max_episode_steps=30)
        return dqn_train.DqnLearner(env, buffer_size=4096, learning_starts=256, batch_size=32, train_freq=4,
                                    gradient_steps=2, target_update_interval=512, seed=seed, track_episodes=False)
    a = make(7)
    losses = []
    res = a.learn(total_timesteps=32 * 40, callback=lambda l: losses.append(float(l._last_loss)))
    assert res["updates"] > 0 and all(math.isfinite(x) for x in losses)
    assert a.buffer.img.dtype == torch.uint8 and a.buffer.size == 32 * 40
    b = make(7)
    b.learn(total_timesteps=32 * 40, stop_at=32 * 20)
    b.save(str(tmp_path / "checkpoint.pt"))
    c = make(1234)
    c.load(str(tmp_path / "checkpoint.pt"))
    c.learn(total_timesteps=32 * 40)
    flat = lambda l: torch.cat([p.detach().reshape(-1) for p in l.trainer.q_net.parameters()])   # noqa: E731
    assert torch.equal(flat(a), flat(c))
    assert torch.equal(a.buffer.img[:a.buffer.size], c.buffer.img[:c.buffer.size])
    assert torch.equal(a.env.img_state, c.env.img_state) and torch.equal(a.env.obs_image, c.env.obs_image)
