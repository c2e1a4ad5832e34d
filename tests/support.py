"""Comparison helpers shared by the test files: numpy and the standard library only, no HIP library."""
import socket

import numpy as np


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def angle_cols(cfg):
    return [4] + [10 + 4 * s + 3 for s in range(cfg.max_observed_food)]


def obs_diff(cfg, a, b):
    """|a - b| with the columns that hold an angle / pi compared on the circle (-1 and +1 are the same heading).
    Strict: a NaN on either side stays NaN, so `d.max() <= TOL` fails on it (golden_util.obs_diff is the lenient one)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    for c in angle_cols(cfg):
        d[..., c] = np.minimum(d[..., c], 2.0 - d[..., c])
    return d


def same_state(a, b):
    """Two (f64, i32) snapshots hold the same values, food rows that are NaN (no food) in both included."""
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def fields_diff(got, want, views, fields):
    """'' when the two record blocks are identical bit for bit, else which of `fields` (names in the dict that
    `views(block)` returns) differ and where first."""
    if np.array_equal(got, want):
        return ""
    g, w = views(np.ascontiguousarray(got)), views(np.ascontiguousarray(want))
    bad = []
    for k in fields:
        ty = np.int64 if g[k].dtype == np.float64 else np.int32
        same = g[k].view(ty) == w[k].view(ty)
        if not same.all():
            i = int(np.argmin(same))
            bad.append(f"{k}: {int((~same).sum())} envs, first env {i}: {g[k][i]!r} != {w[k][i]!r}")
    return "; ".join(bad)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
