"""TEST INFRASTRUCTURE -- CPU restatement of the reference's image observation (TrajectoryPlannerEnvironmentImgsReward1).

What the reference does (paths relative to src/pkg_dqn/environment/): ``components/ext_obsv_image.py`` draws the padded
boundary (255) and the padded obstacle outlines (0) with ``cv2.fillPoly`` at ``down_sample`` x the final size, halves
the result with ``cv2.resize`` and stacks a constant distance field as the third channel; ``variants/imgs_reward1.py``
puts it next to the internal observation and reward of the ray variant.

OpenCV is not a dependency of this project, so its rasteriser is restated here.  The rule, **unpinned** against
OpenCV (``tests/tools/raster_pin.py`` records real ``cv2`` output where OpenCV is installed and compares):

1. Vertices: ``np.int32(original_size * (scale * (R @ (v - p)) + center))`` with ``R = [[s, -c], [c, s]]``,
   ``c, s = cos, sin(theta - angle)`` -- truncation toward zero; written element by element here (a numpy ``@`` may run
   through BLAS with fused multiply-adds), vertices clamped to +-2^20 px.
2. Outline: every edge v[k] -> v[k + 1], horizontal ones included, is drawn as an 8-connected line: ``cv2.clipLine``
   (Cohen-Sutherland, intersections in double, truncated; the first end point is moved before the second is clipped),
   then ``LineIterator(leftToRight=True)``: walk from the left end along the major axis (x on ties), step the minor axis
   while the error term ``err`` (start ``major - 2 minor``) is negative.
3. Scanline fill: an edge with ``y0 != y1`` is active on rows ``y_upper <= y < y_lower``; its x is kept in 16.16 fixed
   point from its upper vertex with the slope ``((x1 - x0) << 16) / (y1 - y0)`` truncated toward zero.  Per row the
   active x values are sorted, paired even-odd, and each pair fills ``[xl >> 16, xr >> 16]`` clipped to the image.
4. ``cv2.resize(INTER_LINEAR)`` at exactly half size on uint8: ``(a + b + c + d + 2) >> 2`` of each 2 x 2 block.
5. Distance field: ext_obsv_image.py:42-50 in numpy, once.

Points where OpenCV releases are known to differ, which the pin tool settles: whether the left end of a fill span is
rounded down (as here) or up, and whether unclipped edges start half a pixel to the right.

The history (ext_obsv_image.py:52-54,66-71): every observation prepends the current outlines and keeps 6 entries; channel
1 uses the oldest.  ``reset()`` clears it.  It is kept here as a list of obstacle clocks.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from oracle import rl_env_numpy as orc

PIX_CLAMP = 1048576.0  # 2^20
HIST = 6


# ------------------------------------------------------------------------------------------------------------------
# rasteriser
# ------------------------------------------------------------------------------------------------------------------
def clip_line(w: int, h: int, x1: int, y1: int, x2: int, y2: int):
    """cv2.clipLine on the rectangle [0, w) x [0, h): (visible, x1, y1, x2, y2)."""
    right, bottom = w - 1, h - 1
    code = lambda x, y: (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8
    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def line_pixels_stepwise(x0: int, y0: int, x1: int, y1: int):
    """LineIterator's error-term walk, one pixel at a time (no clipping): list of (x, y)."""
    dx, dy = x1 - x0, y1 - y0
    if dx < 0:
        x0, y0, dx, dy = x1, y1, -dx, -dy
    sy = -1 if dy < 0 else 1
    ady = abs(dy)
    ymajor = ady > dx
    major, minor = (ady, dx) if ymajor else (dx, ady)
    err = major - 2 * minor
    x, y, out = x0, y0, []
    for _ in range(major + 1):
        out.append((x, y))
        mv = err < 0
        err += -2 * minor + (2 * major if mv else 0)
        if ymajor:
            y += sy
            x += 1 if mv else 0
        else:
            x += 1
            y += sy if mv else 0
    return out


def line_pixels(x0: int, y0: int, x1: int, y1: int):
    """The same walk in closed form: the minor offset after i steps is ceil((2 minor i - major) / (2 major))."""
    dx, dy = x1 - x0, y1 - y0
    if dx < 0:
        x0, y0, dx, dy = x1, y1, -dx, -dy
    sy = -1 if dy < 0 else 1
    ady = abs(dy)
    ymajor = ady > dx
    major, minor = (ady, dx) if ymajor else (dx, ady)
    i = np.arange(major + 1, dtype=np.int64)
    m = (2 * minor * i + major - 1) // (2 * major) if major > 0 else np.zeros(1, dtype=np.int64)
    if ymajor:
        return x0 + m, y0 + sy * i
    return x0 + i, y0 + sy * m


def fill_poly(img: np.ndarray, pts: np.ndarray, color: int) -> None:
    """cv2.fillPoly(img, [pts], color) with LINE_8, shift 0, as restated in the module docstring (in place)."""
    h, w = img.shape
    pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
    n = len(pts)
    edges = []
    for k in range(n):
        (xa, ya), (xb, yb) = pts[k], pts[(k + 1) % n]
        ok, cx0, cy0, cx1, cy1 = clip_line(w, h, xa, ya, xb, yb)
        if ok:
            xs, ys = line_pixels(cx0, cy0, cx1, cy1)
            keep = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
            img[ys[keep], xs[keep]] = color
        if ya != yb:
            num = (xb - xa) * 65536
            den = yb - ya
            q = abs(num) // abs(den)
            dx = q if (num >= 0) == (den > 0) else -q      # C division: truncation toward zero
            xu, yu, yl = (xa, ya, yb) if ya < yb else (xb, yb, ya)
            edges.append((xu * 65536, yu, yl, dx))
    for y in range(h):
        xs = sorted(x0 + (y - yu) * dx for x0, yu, yl, dx in edges if yu <= y < yl)
        for i in range(0, len(xs) - 1, 2):
            xl, xr = xs[i] >> 16, xs[i + 1] >> 16
            if xl < w and xr >= 0:
                img[y, max(xl, 0):min(xr, w - 1) + 1] = color


def resize_half(img: np.ndarray) -> np.ndarray:
    """cv2.resize(img, (w // 2, h // 2)) with INTER_LINEAR on uint8 at exactly half size."""
    a = img.astype(np.int32)
    s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


def distance_field(width: int, height: int, scale_x: float, scale_y: float, center_x: float, center_y: float) -> np.ndarray:
    """ext_obsv_image.py:42-50 (uint8 [height, width])."""
    w = (width - 1) / (scale_x * width)
    h = (height - 1) / (scale_y * height)
    xrange = np.linspace(-w * center_x, w * (1 - center_x), width)
    yrange = np.linspace(-h * center_y, h * (1 - center_y), height)
    x, y = np.meshgrid(xrange, yrange)
    distance = 2 / (1 + np.exp(-2 * np.sqrt(x ** 2 + y ** 2) / 10)) - 1   # components/utils.py:10-15
    distance = distance - np.min(distance)
    return (255.5 * (1 - distance / np.max(distance))).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------
# the image observation
# ------------------------------------------------------------------------------------------------------------------
class ImageParams:
    def __init__(self, width=54, height=54, scale_x=1 / 18, scale_y=1 / 18, down_sample=2, center_x=0.5, center_y=0.3,
                 angle=0.0):
        self.width, self.height, self.down_sample = int(width), int(height), down_sample
        self.scale_x, self.scale_y, self.center_x, self.center_y, self.angle = scale_x, scale_y, center_x, center_y, angle


def obstacle_world(ob: Dict, clock: float) -> np.ndarray:
    """Padded outline of one obstacle at ``clock``: position + R(rotation) * node, element by element."""
    px, py, rot = orc.keyframe_pose(ob["time_steps"], ob["keyframes"], ob["interp"], ob["offset"], clock)
    c, s = math.cos(rot), math.sin(rot)
    nodes = np.asarray(ob["padded_nodes"], dtype=np.float64)
    return np.stack([px + (c * nodes[:, 0] - s * nodes[:, 1]), py + (s * nodes[:, 0] + c * nodes[:, 1])], axis=1)


def to_pixels(world: np.ndarray, pose, ip: ImageParams):
    """(int pixels [n, 2], distance of every coordinate before the clamp and the truncation to the nearest value where
    its pixel would change [n, 2]).

    Away from the clamp that is the nearest integer.  A coordinate beyond +-2^20 px clamps to 2^20 on either side of a
    last-ulp difference, so only its distance to the clamp itself counts (the clamped value would otherwise always
    count as exactly on an integer)."""
    c, s = math.cos(pose[2] - ip.angle), math.sin(pose[2] - ip.angle)
    dx, dy = world[:, 0] - pose[0], world[:, 1] - pose[1]
    px = (2.0 * ip.width) * (ip.scale_x * (s * dx - c * dy) + ip.center_x)
    py = (2.0 * ip.height) * (ip.scale_y * (c * dx + s * dy) + ip.center_y)
    raw = np.stack([px, py], axis=1)
    near = np.where(np.abs(raw) >= PIX_CLAMP, np.abs(raw) - PIX_CLAMP, np.abs(raw - np.round(raw)))
    return np.trunc(np.clip(raw, -PIX_CLAMP, PIX_CLAMP)).astype(np.int64), near


def render_pair(spec: Dict, pose, clock0: float, clock1: float, ip: ImageParams, dfield: Optional[np.ndarray] = None,
                eps: float = 1e-9):
    """uint8 [3, H, W] of robot ``pose`` (x, y, theta) with the obstacles at clocks ``clock0`` (channel 0) and ``clock1``
    (channel 1); second value: True when a vertex lies within ``eps`` of an integer pixel before truncation."""
    if ip.down_sample != 2:
        raise ValueError("only down_sample = 2 is restated")
    W2, H2 = 2 * ip.width, 2 * ip.height
    img0 = np.zeros((H2, W2), dtype=np.uint8)
    bpix, bnear = to_pixels(np.asarray(spec["boundary_padded"], dtype=np.float64), pose, ip)
    ambiguous = bool((bnear < eps).any())
    fill_poly(img0, bpix, 255)
    img1 = img0.copy()
    for img, clock in ((img0, clock0), (img1, clock1)):
        for ob in spec["obstacles"]:
            pix, near = to_pixels(obstacle_world(ob, clock), pose, ip)
            ambiguous |= bool((near < eps).any())
            fill_poly(img, pix, 0)
    if dfield is None:
        dfield = distance_field(ip.width, ip.height, ip.scale_x, ip.scale_y, ip.center_x, ip.center_y)
    return np.stack([resize_half(img0), resize_half(img1), dfield]), ambiguous


class ImageHistory:
    """``ImageObservation.obstacles`` as obstacle clocks: push one per observation, keep 6, channel 1 = the oldest."""

    def __init__(self):
        self.clocks = []

    def reset(self):
        self.clocks = []

    def push(self, clock: float):
        self.clocks = [clock] + self.clocks[:HIST - 1]
        return clock, self.clocks[-1]


class OracleImgsEnv:
    """``TrajectoryPlannerEnvironmentImgsReward1`` for ONE environment: ``OracleRaysEnv`` for the robot, obstacles,
    internal observation, reward and flags; the image observation above for ``external``."""

    def __init__(self, spec: Dict, image: Optional[ImageParams] = None, **kw):
        self.ip = image or ImageParams()
        self.dfield = distance_field(self.ip.width, self.ip.height, self.ip.scale_x, self.ip.scale_y, self.ip.center_x,
                                     self.ip.center_y)
        self.hist = ImageHistory()
        self.rays = orc.OracleRaysEnv(spec, **kw)
        self.spec = spec
        self.reset()

    def image(self, pose=None, clock=None):
        """Observe: push the history and draw (``pose`` / ``clock`` default to the oracle's own state)."""
        pose = self.rays.state[:3] if pose is None else pose
        clock = self.rays.time if clock is None else clock
        c0, c1 = self.hist.push(clock)
        img, self.last_ambiguous = render_pair(self.spec, pose, c0, c1, self.ip, self.dfield)
        return img

    def reset(self):
        self.hist.reset()
        o = self.rays.reset()
        return {"internal": o["internal"], "external": self.image()}

    def step(self, action: Optional[int]):
        o, r, done, info = self.rays.step(action)
        return {"internal": o["internal"], "external": self.image()}, r, done, info
