"""Inputs and exact references for the tests of the robot kernels' fp64 primitives (csrc/salp_fp64_math.h):
tests/test_robot_math.py holds the host twin to mpmath, tests/test_gpu_robot_math.py holds the device to the host twin
on the same inputs, subsampled.  Errors are absolute: sin and cos are bounded by 1, and relative error means nothing at
their zeros."""
import math

import mpmath
import numpy as np

PREC = 256                      # bits of the mpmath references
ULP1 = 2.0 ** -52               # one ulp of 1
STEPS = 1460                    # Euler steps of the longest cycle: the 14.6 s cut at dt = 0.01
SMALL_RANGES = (math.pi, 1e2, 1e4, 1e6, 1e8, 1e9)
CHAIN_STARTS = (0.3, -2.9, 123.456, 1e4 + 0.7)


def sincos_error(x, s, c):
    """max(|s - sin x|, |c - cos x|) per element, x taken as the exact double it is."""
    out = np.empty(len(x))
    with mpmath.workprec(PREC):
        for i, (xi, si, ci) in enumerate(zip(x, s, c)):
            cr, sr = mpmath.cos_sin(mpmath.mpf(float(xi)))
            out[i] = max(abs(mpmath.mpf(float(si)) - sr), abs(mpmath.mpf(float(ci)) - cr))
    return out


def small_range_points(limit, count=20000):
    rng = np.random.default_rng([1, int(limit)])
    return rng.uniform(-limit, limit, count)


def _near(v):
    """v (a double) and the points within 2^-20 ... 2^-52 relative of it on both sides, and its nearest neighbours."""
    pts = [v]
    for j in range(20, 53):
        pts += [v * (1.0 + 2.0 ** -j), v * (1.0 - 2.0 ** -j)]
    lo = hi = v
    for _ in range(3):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        pts += [float(lo), float(hi)]
    return pts


def _multiples():
    rng = np.random.default_rng(2)
    ks = set(range(-4, 5)) | set(range(5, 41)) | {int(k) for k in rng.integers(41, 20000, 150)} | {19999, 20000}
    ks |= {-k for k in list(ks)[::3]}
    return sorted(ks)


def small_edge_points():
    """Next to every zero of sin or cos (k pi/2, |k| <= 4 and k up to 2e4), on both sides of every quadrant switch of the
    reduction ((k + 1/2) pi/2, where rint(x 2/pi) steps), and +-0."""
    pts = [0.0, -0.0]
    with mpmath.workprec(PREC):
        for k in _multiples():
            if k:
                pts += _near(float(k * mpmath.pi / 2))
            pts += _near(float((k + mpmath.mpf(1) / 2) * mpmath.pi / 2))
    return np.array(pts)


def euler_points(count=20000):
    """Log-uniform 1e8 < |x| <= 1e15 in both signs: every group of 64 folds."""
    rng = np.random.default_rng(3)
    return 10.0 ** rng.uniform(8.0001, 15.0, count) * rng.choice([-1.0, 1.0], count)


def euler_switch_points(fold_above):
    """Three groups of 64 around the fold switch: [0] all at or just below it (no fold), [1] small angles and angles next
    to the switch with one lane above it (the whole group folds), [2] all just above it."""
    rng = np.random.default_rng(4)
    t = fold_above
    below = np.concatenate([[t, -t, np.nextafter(t, 0), -np.nextafter(t, 0)], rng.uniform(-t, t, 60)])
    mixed = np.concatenate([[np.nextafter(t, np.inf)], [t, -t, 0.0, 1.0, -3.0, 1e4, -1e6], rng.uniform(-t, t, 56)])
    above = np.concatenate([[np.nextafter(t, np.inf), -np.nextafter(t, np.inf)], rng.uniform(t, 1.001 * t, 62) * rng.choice([-1.0, 1.0], 62)])
    return np.concatenate([below, mixed, above])


def rotate_points(limit, count=20000):
    """theta over the circle, (s, c) = correctly rounded sin / cos of it, d within the switch threshold (a quarter of them
    at it).  Returns theta, s, c, d."""
    rng = np.random.default_rng(5)
    th = rng.uniform(-math.pi, math.pi, count)
    d = rng.uniform(-limit, limit, count)
    d[::4] = np.where(d[::4] < 0, -limit, limit)
    s, c = np.empty(count), np.empty(count)
    with mpmath.workprec(PREC):
        for i, t in enumerate(th):
            cr, sr = mpmath.cos_sin(mpmath.mpf(float(t)))
            s[i], c[i] = float(sr), float(cr)
    return th, s, c, d


def rotate_error(th, d, s, c):
    """Against sin / cos of the exact theta + d."""
    out = np.empty(len(th))
    with mpmath.workprec(PREC):
        for i in range(len(th)):
            cr, sr = mpmath.cos_sin(mpmath.mpf(float(th[i])) + mpmath.mpf(float(d[i])))
            out[i] = max(abs(mpmath.mpf(float(s[i])) - sr), abs(mpmath.mpf(float(c[i])) - cr))
    return out


def chain_inputs(limit, steps=STEPS, seeds=6):
    """[1 + steps][n]: row 0 the start angles, then the increments.  Per start angle: constant at +-limit, alternating
    +-limit, `seeds` draws uniform within +-limit, and `seeds` draws around 1e-3 rad (the kernel's normal regime).
    Padded to whole groups of 64 with copies of the first chains."""
    cols = []
    k = np.arange(steps)
    for x0 in CHAIN_STARTS:
        rng = np.random.default_rng([6, int(abs(x0) * 10)])
        pats = [np.full(steps, limit), np.full(steps, -limit), np.where(k % 2 == 0, limit, -limit)]
        pats += [rng.uniform(-limit, limit, steps) for _ in range(seeds)]
        pats += [rng.uniform(0.5e-3, 1.5e-3, steps) * rng.choice([-1.0, 1.0]) for _ in range(seeds)]
        cols += [np.concatenate([[x0], p]) for p in pats]
    a = np.stack(cols, axis=1)
    pad = -a.shape[1] % 64
    return np.concatenate([a, a[:, :pad]], axis=1)


def chain_errors(inp, s, c, angle):
    """(a) against sin / cos of the exact x0 + sum d, (b) against sin / cos of the accumulated double `angle`."""
    n = inp.shape[1]
    ea = np.empty(n)
    with mpmath.workprec(PREC):
        for i in range(n):
            exact = mpmath.fsum(mpmath.mpf(float(v)) for v in inp[:, i])
            cr, sr = mpmath.cos_sin(exact)
            ea[i] = max(abs(mpmath.mpf(float(s[i])) - sr), abs(mpmath.mpf(float(c[i])) - cr))
    return ea, sincos_error(angle, s, c)


def accumulation_bound(inp):
    """steps * ulp(max |angle|) / 2: the rounding of `eul += d` over the chain, which no carried scheme can remove."""
    path = np.abs(np.cumsum(inp, axis=0)).max(axis=0)
    return (inp.shape[0] - 1) * np.spacing(path) / 2


def mixed_group_inputs(limit, steps=40, groups=3, lane=17, group=1):
    """`groups` groups of 64 chains with increments around 1e-3; in the variant `big` one lane of one group gets an
    increment above the threshold on the LAST step.  Returns (plain, big)."""
    rng = np.random.default_rng(7)
    n = 64 * groups
    plain = np.concatenate([rng.uniform(-200.0, 200.0, (1, n)), rng.uniform(-2e-3, 2e-3, (steps, n))])
    big = plain.copy()
    big[steps, 64 * group + lane] = 1.2 * limit
    return plain, big


def random_robot_params(rng, n):
    """[12, n] robot parameter columns: the defaults scaled by uniform(0.5, 1.5), kept consistent (drag min < max, the
    contraction at most half the length) — the random parameter box of the trajectory tests."""
    from underwater_swimmer_rl_amd.robot_compare import ROBOT_PARAM_NAMES, robot_params
    d = robot_params(1, "cpu").numpy()[:, 0]
    P = d[:, None] * rng.uniform(0.5, 1.5, (12, n))
    j = {name: i for i, name in enumerate(ROBOT_PARAM_NAMES)}
    lo, hi = np.minimum(P[j["drag_coefficient_min"]], P[j["drag_coefficient_max"]]), np.maximum(P[j["drag_coefficient_min"]], P[j["drag_coefficient_max"]])
    P[j["drag_coefficient_min"]], P[j["drag_coefficient_max"]] = lo, hi + 1e-3
    P[j["max_contraction"]] = np.minimum(P[j["max_contraction"]], 0.5 * P[j["init_length"]])
    return P
