"""Arguments for the tests of ``csrc/per_pow.hpp`` (``libm_pow``) on the host (tests/test_per_pow_host.py) and,
through the priorities of ``update``, on the device (tests/test_gpu_per.py), with a CENSUS of what they reach.

The census is computed here from the index formulas written in per_pow.hpp, not by the code under test:

* log interval   ``i = ((bits(x) - 0x3fe6955500000000) >> 45) & 127`` -- exact integer arithmetic;
* exp entry      ``ki & 127`` with ``ks = ehi * EXP_INVLN2N + EXP_SHIFT``, i.e. ``rint(ehi * 128 / ln 2) & 127``.  ``ehi`` is the
  library's own rounded ``y log x``; here it is ``y * log(x)`` of numpy, a few ulps from it, so a point is counted for an entry
  only when the product lies further than 0.01 from a rounding boundary (``decidable``);
* the ways out  ``x`` zero / subnormal / not a positive finite number, ``y`` zero of either sign / outside 2^-65 <= |y| < 2^63,
  ``|y log x| < 2^-54`` (the early return, covered) and ``|y log x| >= 512`` (not covered), the last two again on numpy's
  ``y * log(x)``: the generator puts no point within a factor 1 +- 1e-6 of either threshold.
"""
from __future__ import annotations

import numpy as np

LOG_OFF = np.uint64(0x3FE6955500000000)
EXP_INVLN2N = float.fromhex("0x1.71547652b82fep+7")
# classes of census()["kind"]
TABLE, TINY, HUGE, X_ZERO, X_SUBNORMAL, X_OTHER, Y_ZERO, Y_NEG_ZERO, Y_RANGE = range(9)
KIND_NAMES = ("table", "tiny", "huge", "x_zero", "x_subnormal", "x_other", "y_zero", "y_neg_zero", "y_range")
# (alpha, epsilon) of the power sweep through ``update`` (tests/test_gpu_per.py)
SWEEP = tuple((a, e) for a in (0.1, 0.5, 0.6, 1.0, 2.0) for e in (1e-6, 1e-2)) + ((1e-3, 2.0 ** -52), (0.6, 0.0))


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def log_interval(x):
    return (((_bits(x) - LOG_OFF) >> np.uint64(45)) & np.uint64(127)).astype(np.int64)


def census(x, y):
    """-> dict(kind [n] (the classes above), covered [n] bool, log [n] interval or -1, exp [n] entry or -1 (-1 also where
    the entry is not decidable), log_intervals / exp_entries: sorted unique lists, kinds: name -> count)."""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    topx = (_bits(x) >> np.uint64(52)).astype(np.int64)                # sign included: a negative x is far above 0x7fe
    topy = ((_bits(y) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    kind = np.full(x.shape, TABLE, np.int64)
    x_ok = (topx >= 1) & (topx <= 0x7FE)
    y_ok = (topy >= 0x3BE) & (topy <= 0x3BE + 0x7F)
    kind[~y_ok] = Y_RANGE
    kind[(y == 0.0) & ~np.signbit(y)] = Y_ZERO
    kind[(y == 0.0) & np.signbit(y)] = Y_NEG_ZERO
    kind[~x_ok] = X_OTHER                                               # x decides first, as in the header's test
    kind[(topx == 0) & (x != 0.0)] = X_SUBNORMAL
    kind[x == 0.0] = X_ZERO
    main = kind == TABLE
    with np.errstate(all="ignore"):
        ehi = np.where(main, y * np.log(np.where(main, x, 1.0)), 0.0)
    kind[main & (np.abs(ehi) < 2.0 ** -54)] = TINY
    kind[main & (np.abs(ehi) >= 512.0)] = HUGE
    near = main & ((np.abs(np.abs(ehi) / 2.0 ** -54 - 1.0) < 1e-6) | (np.abs(np.abs(ehi) / 512.0 - 1.0) < 1e-6))
    assert not near.any(), "a generated point lies on a threshold of the covered range"
    table = kind == TABLE
    z = ehi * EXP_INVLN2N
    k = np.rint(z)
    decidable = table & (np.abs(z - k) < 0.49)
    log_i = np.where(table | (kind == TINY) | (kind == HUGE), log_interval(x), -1)
    exp_i = np.where(decidable, k.astype(np.int64) & 127, -1)
    return dict(kind=kind, covered=table | (kind == TINY), log=log_i, exp=exp_i,
                log_intervals=sorted(set(log_i[log_i >= 0].tolist())), exp_entries=sorted(set(exp_i[exp_i >= 0].tolist())),
                kinds={name: int(np.sum(kind == c)) for c, name in enumerate(KIND_NAMES)})


def mantissas(rng, intervals, low_bits=45):
    """Doubles in [0.70, 1.41) whose log interval is ``intervals[j]``: bits(x) = offset + (interval << 45) + low, where of the
    45 bits of ``low`` the top ``low_bits`` are random and the rest zero (low_bits = 16: x is a float32 value)."""
    intervals = np.asarray(intervals, np.uint64)
    low = rng.integers(0, 1 << low_bits, len(intervals), dtype=np.uint64) << np.uint64(45 - low_bits)
    return (LOG_OFF + (intervals << np.uint64(45)) + low).view(np.float64)


def td_errors(n=4096, seed=4096):
    """``n`` float32 TD errors: row r has log interval r mod 128 (all 128, 32 times over), binary exponent spread over -60 .. 60
    by r // 128, alternating sign; rows 0, 1 and 2 are exact 0, 1 and -1."""
    rng = np.random.default_rng(seed)
    r = np.arange(n)
    groups = max(1, (n + 127) // 128)
    expo = np.rint(-60.0 + (r // 128) * (120.0 / max(1, groups - 1))).astype(np.int64)
    td = np.ldexp(mantissas(rng, r % 128, low_bits=16), expo) * np.where(r % 2 == 0, 1.0, -1.0)
    td[:3] = (0.0, 1.0, -1.0)
    out = td.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), td)                 # every value IS a float32
    return out


def priority_arguments(td, alpha, epsilon):
    """(x, y) of the leaves ``update`` writes: x = |td| + epsilon in float64 from the float32 td."""
    x = np.abs(np.asarray(td, np.float32).astype(np.float64)) + float(epsilon)
    return x, np.full(x.shape, float(alpha))


def host_arguments(seed=20261020):
    """The (x, y) of the host test: float64 [n] each, n about 1.6 * 10^6, deterministic.

    1  16 exponents y between -1 and 3 on x = 2^e * m, e = -100 .. 100, m stepping through the 128 log intervals (random low bits);
    2  x within a few ulps of 1 with y chosen so that |y log x| runs over 2^-83 .. 2^-43, both sides of the early return;
    3  the priorities |float32| + epsilon of the power sweep (the TD errors of :func:`td_errors` and random float32 values);
    4  the weights' (n p / total)^-beta and Adam's beta^t for t = 1 .. 2000 and up to 10^6;
    5  every way out of the covered range that a setting can produce;
    6  arguments whose exact power lies on a rounding boundary."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []

    def put(x, y):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        xs.append(x.reshape(-1).copy()); ys.append(y.reshape(-1).copy())

    # 1
    for y in (-1.0, -0.7, -0.6, -0.5, -0.4, -0.3, 1e-3, 0.1, 0.3, 0.5, 0.6, 0.7, 1.0, 1.5, 2.0, 3.0):
        e = np.repeat(np.arange(-100, 101), 128)
        put(np.ldexp(mantissas(rng, np.tile(np.arange(128), 201)), e), y)
    # 2: log(1 + j ulp) = j 2^-52 (above 1) or -j 2^-53 (below); y = 2^-s
    j = rng.integers(1, 64, 100_000)
    above = rng.random(100_000) < 0.5
    x = np.where(above, 1.0 + j * 2.0 ** -52, 1.0 - j * 2.0 ** -53)
    put(x, np.ldexp(rng.uniform(1.0, 2.0, 100_000), -rng.integers(0, 37, 100_000)) * np.where(rng.random(100_000) < 0.5, 1.0, -1.0))
    put([1.0, 1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53], [0.3, -0.4, 1e-3, 1e-3])
    # 3
    td = td_errors()
    wide = (rng.standard_normal(60_000) * np.exp(rng.uniform(-12.0, 6.0, 60_000))).astype(np.float32)
    for alpha, epsilon in SWEEP + ((0.3, 1e-3),):
        put(*priority_arguments(td, alpha, epsilon))
        put(*priority_arguments(wide, alpha, epsilon))
    # 4
    for beta in (0.4, 0.6, 1.0):
        put(np.exp(rng.uniform(-14.0, 14.0, 20_000)), -beta)
    for beta in (0.9, 0.999, 0.5, 0.99, 0.9999, 0.8):
        put(beta, np.concatenate([np.arange(1.0, 2001.0), [10.0 ** 4, 10.0 ** 5, 10.0 ** 6]]))
    # 5: x = 0 (epsilon = 0 and td = 0; beta1 = 0), y = +-0 (alpha = 0, beta = 0, -beta = -0), a subnormal x (epsilon = 1e-310),
    # |y log x| >= 512 (the bias correction at a million steps, 0.5^999 from a checkpoint)
    put([0.0, 0.0, 0.0, 1.5, 1e-3, 0.25, 2.0, 1e-310, 5e-324, 0.999, 0.5, 0.99, 0.8],
        [0.6, 1.0, 10.0 ** 6, 0.0, 0.0, -0.0, -0.0, 0.6, 0.3, 10.0 ** 6, 999.0, 10.0 ** 6, 10.0 ** 6])
    # 6: results that lie exactly on a rounding boundary -- x an odd 27-bit integer and y = 2 (x^2 has 53 or 54 bits), an odd
    # 18-bit integer and y = 3 -- where the sign of the algorithm's own last error (2^-68) decides the bit: what the random
    # arguments above are too few to notice, these notice
    m27 = (rng.integers(2 ** 25, 2 ** 26, 150_000) * 2 + 1).astype(np.float64)
    put(np.ldexp(m27, rng.integers(-60, 8, 150_000)), 2.0)
    m18 = (rng.integers(2 ** 16, 2 ** 17, 50_000) * 2 + 1).astype(np.float64)
    put(np.ldexp(m18, rng.integers(-40, 8, 50_000)), 3.0)
    return np.concatenate(xs), np.concatenate(ys)
