"""Numpy twin of csrc/dqngpu.hip (include/mpcgpu_dqn.h): the same float32 operations in the stated orders.

Vector operations run over independent outputs (rows, units, parameters); every SUMMED index is a Python loop, so the order
of each sum is the header's.  Sampling is Python-integer arithmetic, the bias corrections are ``beta ** t`` in float64."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

OBS, HID, ACT, NP = 46, 16, 9, 1177
OFF_W0, OFF_B0, OFF_W1, OFF_B1, OFF_W2, OFF_B2 = 0, 736, 752, 1008, 1024, 1168
LANES = 256
STATE_T, STATE_FLOATS = 4708, 4712
F = np.float32
_MASK = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def split(theta):
    """Flat parameter vector -> (W0 [16, 46], b0, W1 [16, 16], b1, W2 [9, 16], b2), views."""
    return (theta[OFF_W0:OFF_B0].reshape(HID, OBS), theta[OFF_B0:OFF_W1], theta[OFF_W1:OFF_B1].reshape(HID, HID),
            theta[OFF_B1:OFF_W2], theta[OFF_W2:OFF_B2].reshape(ACT, HID), theta[OFF_B2:NP])


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def sample_rows(seed: int, serial: int, n: int, size: int) -> np.ndarray:
    """Rows of the minibatch of step ``serial`` of stream ``seed`` on a buffer of ``size`` rows."""
    key = mix64((seed + _G * serial) & _MASK)
    return np.array([(mix64((key + _G * (i + 1)) & _MASK) * size) >> 64 for i in range(n)], dtype=np.int64)


def dense(W, b, x, relu):
    acc = np.broadcast_to(b, (x.shape[0], W.shape[0])).astype(F)
    for k in range(W.shape[1]):
        acc = acc + W[None, :, k] * x[:, k, None]
    return np.where(acc > 0, acc, F(0)).astype(F) if relu else acc


def network(theta, x):
    W0, b0, W1, b1, W2, b2 = split(theta)
    h1 = dense(W0, b0, x, True)
    h2 = dense(W1, b1, h1, True)
    return h1, h2, dense(W2, b2, h2, False)


def fold(slots):
    s = np.zeros(LANES, F)
    s[:len(slots)] = slots
    h = LANES // 2
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def gradient(theta, target, obs, next_obs, actions, rewards, dones, weights: Optional[np.ndarray], gamma, double_q):
    """-> (unclipped mean gradient [1177], loss, delta [n]), all float32."""
    theta, target = np.asarray(theta, F), np.asarray(target, F)
    obs, next_obs = np.asarray(obs, F), np.asarray(next_obs, F)
    rewards, dones = np.asarray(rewards, F), np.asarray(dones, F)
    n = obs.shape[0]
    rows = np.arange(n)
    _, _, qt = network(target, next_obs)
    scan = network(theta, next_obs)[2] if double_q else qt
    top, next_v = scan[:, 0].copy(), qt[:, 0].copy()
    for a in range(1, ACT):
        better = scan[:, a] > top
        top = np.where(better, scan[:, a], top)
        next_v = np.where(better, qt[:, a], next_v)
    h1, h2, q = network(theta, obs)
    act = np.clip(np.asarray(actions, np.int64), 0, ACT - 1)
    y = rewards + ((F(1) - dones) * F(gamma)) * next_v
    d = (y - q[rows, act]).astype(F)
    e = np.abs(d)
    l = np.where(e < 1, (F(0.5) * e) * e, e - F(0.5)).astype(F)
    c = np.where(e < 1, -d, np.where(d > 0, F(-1), F(1))).astype(F)
    if weights is not None:
        w = np.asarray(weights, F)
        l, c = w * l, w * c
    loss = fold(l) / F(n)
    g = (c / F(n)).astype(F)
    W0, b0, W1, b1, W2, b2 = split(theta)
    dz2 = np.where(np.arange(ACT)[None, :] == act[:, None], g[:, None], F(0)).astype(F)
    dz1 = np.where(h2 > 0, W2[act] * g[:, None], F(0)).astype(F)
    dh1 = np.zeros((n, HID), F)
    for j in range(HID):
        dh1 = dh1 + W1[None, j, :] * dz1[:, j, None]
    dz0 = np.where(h1 > 0, dh1, F(0)).astype(F)
    grad = np.zeros(NP, F)
    gW0, gb0, gW1, gb1, gW2, gb2 = split(grad)
    for i in range(n):
        gW0 += dz0[i][:, None] * obs[i][None, :]
        gb0 += dz0[i]
        gW1 += dz1[i][:, None] * h1[i][None, :]
        gb1 += dz1[i]
        gW2 += dz2[i][:, None] * h2[i][None, :]
        gb2 += dz2[i]
    return grad, F(loss), d


def bias_corrections(t: int, lr, beta1, beta2):
    """(step size, root of the second correction) as float32, formed in float64 from the step count."""
    bc1, bc2 = 1.0 - beta1 ** float(t), 1.0 - beta2 ** float(t)
    return F(lr / bc1), F(math.sqrt(bc2))


def apply(theta, m, v, t, grad, scale=1.0, lr=1e-4, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """Clip and Adam -> (theta, m, v, t + 1); the inputs are left alone."""
    theta, m, v = np.asarray(theta, F), np.asarray(m, F), np.asarray(v, F)
    g = np.asarray(grad, F) * F(scale)
    sq = np.zeros(5 * LANES, F)
    sq[:NP] = g * g
    lane = np.zeros(LANES, F)
    for c in range(5):
        lane = lane + sq[c * LANES:(c + 1) * LANES]
    norm = np.sqrt(fold(lane))
    ratio = F(max_grad_norm) / (norm + F(1e-6))
    g = g * (ratio if ratio < 1 else F(1))
    t = int(t) + 1
    step, root = bias_corrections(t, lr, beta1, beta2)
    m = F(beta1) * m + F(1.0 - beta1) * g
    v = F(beta2) * v + F(1.0 - beta2) * (g * g)
    theta = theta - step * (m / (np.sqrt(v) / root + F(eps)))
    return theta.astype(F), m.astype(F), v.astype(F), t


class Twin:
    """The state block and the four entries."""

    def __init__(self, theta, target=None, lr=1e-4, gamma=0.98, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8,
                 double_q=False):
        self.theta = np.array(theta, F)
        self.target = self.theta.copy() if target is None else np.array(target, F)
        self.m, self.v, self.t = np.zeros(NP, F), np.zeros(NP, F), 0
        self.gamma, self.double_q = gamma, double_q
        self.adam = dict(lr=lr, max_grad_norm=max_grad_norm, beta1=beta1, beta2=beta2, eps=eps)

    def grad(self, obs, next_obs, actions, rewards, dones, weights=None):
        return gradient(self.theta, self.target, obs, next_obs, actions, rewards, dones, weights, self.gamma, self.double_q)

    def apply(self, grad, scale=1.0):
        self.theta, self.m, self.v, self.t = apply(self.theta, self.m, self.v, self.t, grad, scale, **self.adam)

    def step(self, obs, next_obs, actions, rewards, dones, weights=None):
        out = self.grad(obs, next_obs, actions, rewards, dones, weights)
        self.apply(out[0])
        return out

    def train(self, buf, size, n, k, seed, serial0):
        """``buf``: dict of the buffer's five arrays -> the K losses."""
        losses = np.zeros(k, F)
        for s in range(k):
            r = sample_rows(seed, serial0 + s, n, size)
            losses[s] = self.step(buf["obs"][r], buf["next_obs"][r], buf["actions"][r], buf["rewards"][r], buf["dones"][r])[1]
        return losses
