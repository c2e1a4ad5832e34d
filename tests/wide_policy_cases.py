"""Policies and shapes shared by the wide in-kernel policy's tests (tests/test_wide_policy_host.py, tests/test_gpu_wide_policy.py).
Needs numpy and `policy.MLPPolicy` / `GaussianPolicy` only.

Weights are DENSE seeded normal draws scaled by gain / sqrt(fan_in), all distinct and non-zero — the rule of
`policy_matrix.dense_policy`, whose constructor stops at 64 units — so that no two words of the re-laid device block can be
exchanged unnoticed; scale is not 1, shift is not 0, the two components differ (`policy_matrix.SCALE` / `SHIFT`)."""
import numpy as np

import gaussian_matrix as gm
import policy_matrix as pm
from underwater_swimmer_rl_amd.policy import GaussianPolicy, MLPPolicy

BOTH_SCHEMES = ((32, 32), (64, 64), (32, 64), (64,))                                   # shapes the narrow scheme runs too
GPU_SHAPES = ((32,), (256,), (32, 32), (64, 64), (96, 160), (256, 32), (32, 256), (256, 256))
GAIN, OUT_GAIN, LS_GAIN = 1.5, 1.5, 0.5


def _draw(sigma, seed, fixed=()):
    rng = np.random.default_rng(seed)
    flat = (rng.standard_normal(sigma.size) * sigma).astype(np.float32)
    fixed = np.asarray(fixed, np.float32)
    while True:
        _, first = np.unique(flat, return_index=True)
        again = np.ones(flat.size, bool)
        again[first] = False
        again |= (flat == 0) | np.isin(flat, fixed)
        if not again.any():
            return flat
        flat[again] = (rng.standard_normal(int(again.sum())) * sigma[again]).astype(np.float32)


def _layers(flat, widths):
    layers, o = [], 0
    for d, h in zip(widths[:-1], widths[1:]):
        layers.append((flat[o:o + h * d].reshape(h, d), flat[o + h * d:o + h * d + h]))
        o += h * d + h
    return layers, o


def _sigma(widths, n_hidden, gain, out_gain):
    s = []
    for li, (d, h) in enumerate(zip(widths[:-1], widths[1:])):
        s += [np.full(h * d, (out_gain if li == n_hidden else gain) / np.sqrt(d)), np.full(h, 0.1)]
    return s


def dense(hidden, A, out="clip", seed=7000, wide=True, gain=GAIN, out_gain=OUT_GAIN):
    """One dense deterministic policy 24 -> hidden -> A."""
    widths = (24,) + tuple(hidden) + (A,)
    flat = _draw(np.concatenate(_sigma(widths, len(hidden), gain, out_gain)), seed + 10 * sum(hidden) + A)
    layers, _ = _layers(flat, widths)
    return MLPPolicy.from_layers(layers, np.array(pm.SCALE[A], np.float32), np.array(pm.SHIFT[A], np.float32), out, wide=wide)


def dense_gauss(hidden, A, seed=7500, wide=True, gain=GAIN, out_gain=OUT_GAIN, ls_gain=LS_GAIN):
    """One dense Gaussian policy; the log-std biases are `gaussian_matrix.B_LS`."""
    widths = (24,) + tuple(hidden) + (A,)
    sigma = _sigma(widths, len(hidden), gain, out_gain) + [np.full(A * widths[-2], ls_gain / np.sqrt(widths[-2]))]
    b_ls = np.asarray(gm.B_LS[A], np.float32)
    flat = _draw(np.concatenate(sigma), seed + 10 * sum(hidden) + A, np.concatenate([b_ls, pm.SCALE[A], pm.SHIFT[A]]))
    layers, o = _layers(flat, widths)
    W_ls = flat[o:o + A * widths[-2]].reshape(A, widths[-2])
    return GaussianPolicy.from_layers(layers, (W_ls, b_ls), np.array(pm.SCALE[A], np.float32), np.array(pm.SHIFT[A], np.float32), wide=wide)


def narrow_twin(p):
    """The same weights as a policy of the narrow scheme (for a shape both accept)."""
    if getattr(p, "gaussian", False):
        return GaussianPolicy(p.layers, p.log_std, p.scale, p.shift)
    return MLPPolicy(p.layers, p.scale, p.shift, p.out)


def rows(n, seed=11):
    """Observation-like rows: values of both signs over a few magnitudes, none zero."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 24)) * rng.choice([0.05, 0.5, 2.0], size=(n, 24))).astype(np.float32)
