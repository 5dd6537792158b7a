"""CPU tests of the image observation (TrajectoryPlannerEnvironmentImgsReward1): the numpy restatement of the rasteriser
on hand-countable cases, the resize, the distance field, the history rule, the image Q-network and the new C-ABI
symbols of the built library (no device needed)."""
import ctypes as C
import importlib
import io
import math
import os
import zipfile

import numpy as np
import torch

from support import image_obs_numpy as im  # noqa: E402
from trajtrack_mpcndqn_rlboost_amd import rl_env
from trajtrack_mpcndqn_rlboost_amd.dqn import ImageQNetwork

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def filled(pts, w=20, h=20):
    img = np.zeros((h, w), dtype=np.uint8)
    im.fill_poly(img, np.asarray(pts), 255)
    return img > 0


def test_axis_aligned_rectangle_includes_its_outline():
    m = filled([(2, 3), (9, 3), (9, 7), (2, 7)])
    assert m.sum() == 8 * 5 and m[3:8, 2:10].all()


def test_triangle_rows():
    m = filled([(0, 0), (8, 0), (0, 8)])
    # row y holds x = 0 .. 8 - y (the hypotenuse is a 45-degree line, its pixels lie on x + y = 8)
    for y in range(9):
        assert np.flatnonzero(m[y]).tolist() == list(range(0, 9 - y)), y
    assert m.sum() == sum(range(1, 10))


def test_concave_polygon_even_odd():
    # a "U": the notch between x = 4 and x = 6 above y = 4 stays empty
    m = filled([(1, 1), (3, 1), (3, 6), (7, 6), (7, 1), (9, 1), (9, 9), (1, 9)])
    assert not m[2:6, 4:7].any()
    assert m[2:9, 1:4].all() and m[2:9, 7:10].all() and m[6:10, 1:10].all()


def test_polygon_far_outside_the_image():
    m = filled([(-10000, -10000), (10000, -10000), (10000, 10000), (-10000, 10000)])
    assert m.all()
    m = filled([(-10000, 5), (10000, 5), (10000, 10000)])
    assert not m[:5].any() and m[5].all()
    assert not filled([(30, 30), (40, 30), (40, 40)]).any()


def test_horizontal_edge_draws_its_line_only():
    m = filled([(2, 4), (12, 4), (7, 4)])   # degenerate: every edge horizontal, no fill, the outline only
    assert np.flatnonzero(m[4]).tolist() == list(range(2, 13)) and m.sum() == 11


def test_vertex_truncation_toward_zero():
    spec = {"boundary_padded": np.array([[0.0, 0.0]]), "obstacles": []}
    ip = im.ImageParams(width=10, height=10, scale_x=1.0, scale_y=1.0, center_x=0.0, center_y=0.0, angle=math.pi / 2)
    # theta - angle = 0: c = 1, s = 0 -> pixel x = 20 * (-dy), pixel y = 20 * dx
    pix, _ = im.to_pixels(np.array([[-0.035, 0.035], [0.035, -0.035]]), (0.0, 0.0, math.pi / 2), ip)
    assert pix.tolist() == [[0, 0], [0, 0]]    # -0.7 px -> 0, not -1; +0.7 -> 0
    pix, _ = im.to_pixels(np.array([[-0.06, -0.06]]), (0.0, 0.0, math.pi / 2), ip)
    assert pix.tolist() == [[1, -1]]           # 1.2 -> 1, -1.2 -> -1


def test_ambiguity_is_measured_before_the_clamp():
    """A coordinate beyond +-2^20 px clamps to the same pixel whatever its last ulp: only its distance to the clamp makes
    it ambiguous, not the integer it is clamped to.  Inside the clamp the distance to the nearest integer counts."""
    ip = im.ImageParams(width=8, height=8, scale_x=1.0, scale_y=1.0, center_x=0.0, center_y=0.0, angle=math.pi / 2)
    # theta - angle = 0: pixel x = 16 * (-dy), pixel y = 16 * dx, every product exact
    world = np.array([[65536.5, 0.0],        # y = 2^20 + 8: clamped, 8 px beyond the clamp
                      [-70000.0, 0.0],       # y = -1 120 000: clamped to -2^20
                      [65536.0, 0.0],        # y = 2^20 exactly: a smaller value would truncate to 2^20 - 1
                      [0.03125, 0.0],        # y = 0.5
                      [100.0, -0.25]])       # y = 1600, x = 4: on integers
    pix, near = im.to_pixels(world, (0.0, 0.0, math.pi / 2), ip)
    assert pix[:, 1].tolist() == [2 ** 20, -2 ** 20, 2 ** 20, 0, 1600] and pix[:, 0].tolist() == [0, 0, 0, 0, 4]
    assert near[:, 1].tolist() == [8.0, 70000.0 * 16 - 2 ** 20, 0.0, 0.5, 0.0]
    eps = 1e-9
    assert (near[:, 1] < eps).tolist() == [False, False, True, False, True]
    # a boundary with clamped corners and no vertex near an integer is drawn and not exempt
    spec = {"boundary_padded": np.array([[-1e5, -1e5 + 0.3], [1e5, -1e5 + 0.3], [1e5, 1e5 + 0.3], [-1e5, 1e5 + 0.3]]),
            "obstacles": []}
    bpix, bnear = im.to_pixels(spec["boundary_padded"], (0.3, 0.2, math.pi / 2), ip)
    assert (np.abs(bpix) == 2 ** 20).all() and (bnear > 1.0).all()
    img, amb = im.render_pair(spec, (0.3, 0.2, math.pi / 2), 0.0, 0.0, ip)
    assert not amb and (img[:2] == 255).all()


def test_closed_form_line_equals_the_stepwise_walk():
    rng = np.random.default_rng(3)
    for _ in range(400):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-40, 40, 4))
        xs, ys = im.line_pixels(x0, y0, x1, y1)
        assert list(zip(xs.tolist(), ys.tolist())) == im.line_pixels_stepwise(x0, y0, x1, y1)


def test_clip_line_on_hand_cases():
    assert im.clip_line(10, 10, -5, 5, 15, 5) == (True, 0, 5, 9, 5)
    assert im.clip_line(10, 10, -5, -5, -1, 20)[0] is False
    ok, x0, y0, x1, y1 = im.clip_line(10, 10, -10, -10, 20, 20)
    assert ok and (x0, y0, x1, y1) == (0, 0, 9, 9)


def test_resize_half_blocks():
    blocks = np.array([[255, 255], [255, 0]], dtype=np.uint8)
    assert im.resize_half(blocks)[0, 0] == 191
    for n, v in zip(range(5), (0, 64, 128, 191, 255)):
        b = np.zeros(4, dtype=np.uint8)
        b[:n] = 255
        assert im.resize_half(b.reshape(2, 2))[0, 0] == v


def test_distance_field_against_the_formula():
    W, H, cx, cy = 54, 54, 0.5, 0.3
    f = im.distance_field(W, H, 1 / 18, 1 / 18, cx, cy)
    assert f.shape == (H, W) and f.dtype == np.uint8
    r, c = np.unravel_index(np.argmax(f), f.shape)
    assert f.max() == 255 and abs(c - cx * (W - 1)) <= 0.5 and abs(r - cy * (H - 1)) <= 0.5
    # decreasing along every ray out of the robot's pixel
    assert (np.diff(f[r, c:].astype(int)) <= 0).all() and (np.diff(f[r:, c].astype(int)) <= 0).all()
    assert (np.diff(f[r, :c + 1].astype(int)) >= 0).all()
    assert np.array_equal(f, rl_env.image_distance_field(W, H, 1 / 18, 1 / 18, cx, cy))


def test_history_rule_on_a_scripted_sequence():
    h = im.ImageHistory()
    seen = []
    for k in range(1, 10):
        seen.append(h.push(float(k)))
    # after the k-th observation channel 1 shows observation max(1, k - 5)
    assert [c1 for _, c1 in seen] == [float(max(1, k - 5)) for k in range(1, 10)]
    h.reset()
    assert h.push(100.0) == (100.0, 100.0)
    assert h.push(101.0) == (101.0, 100.0)


def test_oracle_imgs_env_runs_and_pushes_history_on_observe_only():
    spec = rl_env.make_map([(0, 0), (10, 0), (10, 10), (0, 10)], [[(4, 4), (6, 4), (6, 6), (4, 6)]],
                           [dict(p1=(2, 8), p2=(8, 8), freq=0.5, rx=0.5, ry=0.3, angle=0.0)],
                           (1.5, 1.5, 0.5, 0.0, 0.0), (8.5, 8.5), [(1.5, 1.5), (8.5, 8.5)])
    env = im.OracleImgsEnv(spec)
    o = env.reset()
    assert o["external"].shape == (3, 54, 54) and np.array_equal(o["external"][0], o["external"][1])
    for a in (0, 1, 2, 3, 4, 5, 6):
        o, *_ = env.step(a)
    assert len(env.hist.clocks) == 6
    env.step(None)
    assert len(env.hist.clocks) == 6 and env.hist.clocks[0] == env.rays.time
    assert set(np.unique(o["external"][:2])) <= {0, 64, 128, 191, 255}


def test_library_exports_the_image_symbols_and_rejects_bad_image_params():
    lib = rl_env._bind(solver_mod.load_library())
    header = open(os.path.join(ROOT, "include", "mpcgpu_env.h")).read()
    for name in ("mpcgpu_env_img_state_doubles", "mpcgpu_env_step_imgs_dev", "mpcgpu_env_step_imgs_autoreset_dev"):
        assert name in rl_env.ENV_EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.mpcgpu_env_img_state_doubles(C.byref(rl_env.image_params())) == 16
    assert lib.mpcgpu_env_img_state_doubles(C.byref(rl_env.image_params(down_sample=3))) < 0
    assert b"down_sample" in lib.mpcgpu_env_last_error()
    assert lib.mpcgpu_env_img_state_doubles(C.byref(rl_env.image_params(width=97))) < 0
    assert lib.mpcgpu_env_img_state_doubles(C.byref(rl_env.image_params(height=7))) < 0
    assert lib.mpcgpu_env_img_state_doubles(None) < 0
    assert lib.mpcgpu_env_img_state_doubles(C.byref(rl_env.image_params(width=8, height=96, angle=1.0, center_x=-3))) == 16


def test_image_qnetwork_matches_sb3_layout_and_loads_an_archive(tmp_path):
    net = ImageQNetwork()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes["features_extractor.extractors.external.cnn.0.weight"] == (32, 3, 8, 8)
    assert shapes["features_extractor.extractors.external.cnn.2.weight"] == (64, 32, 4, 4)
    assert shapes["features_extractor.extractors.external.cnn.4.weight"] == (64, 64, 3, 3)
    assert shapes["features_extractor.extractors.external.linear.0.weight"] == (256, 576)
    assert shapes["q_net.0.weight"] == (64, 270) and shapes["q_net.2.weight"] == (64, 64) and shapes["q_net.4.weight"] == (9, 64)
    torch.manual_seed(0)
    src = ImageQNetwork()
    sd = {"q_net." + k: v for k, v in src.state_dict().items()}
    sd.update({"q_net_target." + k: torch.zeros_like(v) for k, v in src.state_dict().items()})
    buf = io.BytesIO()
    torch.save(sd, buf)
    path = tmp_path / "img_model.zip"
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
    got = ImageQNetwork.from_sb3_zip(str(path))
    obs = {"external": torch.randint(0, 256, (4, 3, 54, 54), dtype=torch.uint8), "internal": torch.randn(4, 14)}
    assert torch.equal(got(obs), src(obs))
    # CombinedExtractor: NatureCNN on external / 255 first, then internal
    feats = src.features_extractor(obs)
    assert torch.equal(feats[:, 256:], obs["internal"])
    assert torch.equal(feats[:, :256], src.features_extractor.extractors["external"](obs["external"].float() / 255.0))


def test_raster_pin_tool_compares_a_recording(tmp_path):
    """tests/tools/raster_pin.py: `compare` runs without cv2 (here on a recording the restatement made of itself)."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import raster_pin as rp
    cases = rp.random_cases(25, 2)
    full, small = [], []
    for W, H, polys in cases:
        img = np.zeros((2 * H, 2 * W), np.uint8)
        im.fill_poly(img, polys[0], 255)
        for p in polys[1:]:
            im.fill_poly(img, p, 0)
        full.append(img.reshape(-1))
        small.append(im.resize_half(img).reshape(-1))
    sizes, lens, verts = rp.pack(cases)
    assert all(np.array_equal(a, b) for (_, _, pa), (_, _, pb) in zip(cases, rp.unpack(sizes, lens, verts)) for a, b in zip(pa, pb))
    small[3] = small[3].copy()
    small[3][0] ^= 1
    path = tmp_path / "rec.npz"
    np.savez(path, sizes=sizes, lens=lens, verts=verts, full=np.concatenate(full), small=np.concatenate(small),
             cv2_version=np.array("test"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "raster_pin.py"), "compare", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "24 of 25 cases equal" in r.stdout and "first mismatch: case 3" in r.stdout
