"""ctypes binding of oracle/libsalp_oracle.so — TEST INFRASTRUCTURE (see oracle/salp_oracle.c).

Imported only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

import native_lib
from native_lib import cint, i32, i64, ptr, u64, vp
from underwater_swimmer_rl_amd._capi import (  # noqa: F401  (the snapshot rows and the info width keep their names here)
    F_X, F_Y, F_VX, F_VY, F_THETA, F_OMEGA, F_NOZZLE, F_WATER, F_ELLIPSE_A, F_ELLIPSE_B, F_FOOD0,
    I_PHASE, I_TIMER, I_EXHALE_DUR, I_SHAPE_HOLD, I_STEPS_SINCE_FOOD, I_FOOD_COLLECTED, I_RNG_COUNTER, I_EPISODE_LENGTH, I_COUNT,
    INFO_COLS)

# rows of OracleVec.placement_counters() (oracle/salp_oracle.h SALP_ORACLE_PC_*)
PC_RESET_PLACED, PC_RESET_FORCED, PC_RESPAWN_PLACED, PC_RESPAWN_FORCED, PC_MAX_VALID_REJECTIONS, PC_COUNT = range(6)

_SO = os.path.join(native_lib.ORACLE_DIR, "libsalp_oracle.so")


# every function of oracle/salp_oracle.h, in header order
PROTOTYPES = {
    "salp_oracle_philox4x32_10": (None, [vp, vp, vp]),
    "salp_oracle_set_threads": (None, [cint]),
    "salp_oracle_get_threads": (cint, []),
    "salp_oracle_create": (cint, [vp, i64, u64, i64, ptr(vp)]),
    "salp_oracle_destroy": (None, [vp]),
    "salp_oracle_obs_dim": (cint, [vp]),
    "salp_oracle_act_dim": (cint, [vp]),
    "salp_oracle_reset": (cint, [vp, vp, vp]),
    "salp_oracle_observe": (cint, [vp, vp]),
    "salp_oracle_step": (cint, [vp] * 9),
    "salp_oracle_rollout": (cint, [vp, vp, i32] + [vp] * 8),
    "salp_oracle_rollout_f64": (cint, [vp, vp, i32, vp, vp, vp, vp]),
    "salp_oracle_get_state": (cint, [vp, vp, vp]),
    "salp_oracle_set_state": (cint, [vp, vp, vp]),
    "salp_oracle_global_step": (i64, [vp]),
    "salp_oracle_set_base_num_food": (cint, [vp, cint]),
    "salp_oracle_get_placement_counters": (cint, [vp, vp]),
    "salp_oracle_clear_placement_counters": (cint, [vp]),
    "salp_oracle_set_placement_limits": (cint, [vp, cint, cint]),
    "salp_oracle_policy_forward": (cint, [vp, i32, i32, vp, vp, i64, vp, vp, vp]),
    "salp_oracle_policy_forward_gaussian": (cint, [vp, i32, i32, vp, vp, i64, vp, vp, vp]),
}


def build_oracle(force: bool = False) -> str:
    """Brings the library up to date; make alone decides whether that takes a compiler (`force` is kept for callers)."""
    return native_lib.make("libsalp_oracle.so")


_lib = None


def lib():
    """_SO and build_oracle are read at call time: tests/test_oracle_sanitizers.py points both at the sanitised build."""
    global _lib
    if _lib is None:
        build_oracle()
        _lib = native_lib.declare(ctypes.CDLL(_SO), PROTOTYPES)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def philox(counter, key):
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    lib().salp_oracle_philox4x32_10(_p(c), _p(k), _p(out))
    return tuple(int(v) for v in out)


def policy_forward(policy, obs, weights=None):
    """The in-kernel policy restated in C in the arithmetic include/salp_vec.h promises (salp_oracle_policy_forward): fp32,
    bias first, one fmaf per input in ascending index order, two roundings behind the output activation.
    `policy`: an `MLPPolicy` (its shape; P >= 1); `weights`: float32 [P, words] in the public layout, default
    `policy.pack()`; obs [..., N, obs_dim], env i of the N belonging to policy i // (N / P).
    Returns u (before the output activation) and a, float32 [..., N, act_dim], and the number of non-zero subnormal values
    formed on the way."""
    return _forward("salp_oracle_policy_forward", policy, obs, weights)


def policy_forward_gaussian(policy, obs, weights=None):
    """The two heads of a `GaussianPolicy` restated in C in the same arithmetic (salp_oracle_policy_forward_gaussian), from
    the public Gaussian layout: `weights` float32 [P, words], default `policy.pack()`; obs as for `policy_forward`.
    Returns m (the mean head) and r (the log-std head's raw sum, before its clamp), float32 [..., N, act_dim], and the number
    of non-zero subnormal values formed on the way."""
    if not getattr(policy, "gaussian", False):
        raise ValueError("policy_forward_gaussian takes a GaussianPolicy")
    return _forward("salp_oracle_policy_forward_gaussian", policy, obs, weights)


def _forward(name, policy, obs, weights):
    x = np.ascontiguousarray(obs, dtype=np.float32)
    P, OD, AD = policy.n_policies, policy.obs_dim, policy.act_dim
    if x.shape[-1] != OD:
        raise ValueError(f"obs rows have {x.shape[-1]} columns, the policy takes {OD}")
    w = np.ascontiguousarray(policy.pack() if weights is None else weights, dtype=np.float32).reshape(P, policy.words)
    policy.check_envs(x.shape[-2])
    lead, N = x.shape[:-2], x.shape[-2]
    g = np.ascontiguousarray(np.moveaxis(x.reshape(-1, P, N // P, OD), 1, 0))           # [P, L, G, OD]
    u = np.empty(g.shape[:-1] + (AD,), np.float32)
    a = np.empty_like(u)
    d, total = policy.desc(), 0
    for k in range(P):
        sub = ctypes.c_int64(0)
        rc = getattr(lib(), name)(ctypes.byref(d), OD, AD, _p(w[k]), _p(g[k]), g[k].size // OD, _p(u[k]), _p(a[k]), ctypes.byref(sub))
        if rc != 0:
            raise RuntimeError(f"{name} failed: {rc}")
        total += sub.value
    back = lambda v: np.ascontiguousarray(np.moveaxis(v, 0, 1)).reshape(lead + (N, AD))
    return back(u), back(a), total


class OracleVec:
    """N reference-faithful CPU envs (fp64, libm), with the HIP library's call shapes."""

    def __init__(self, cfg, n_envs: int, seed: int = 0, env_index_base: int = 0, threads: int = 1):
        self.cfg = cfg
        self.n = int(n_envs)
        self.obs_dim = cfg.obs_dim
        self.act_dim = cfg.act_dim
        self.F = cfg.num_food_items
        self._c = cfg.to_c()
        self._h = ctypes.c_void_p()
        lib().salp_oracle_set_threads(int(threads))
        rc = lib().salp_oracle_create(ctypes.byref(self._c), self.n, seed, env_index_base,
                                      ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(f"salp_oracle_create failed: {rc}")

    def set_base_num_food(self, k):
        if lib().salp_oracle_set_base_num_food(self._h, int(k)) != 0:
            raise ValueError(f"base_num_food_items {k} out of range")

    def placement_counters(self):
        """int64 [PC_COUNT, n] (oracle/salp_oracle.h SALP_ORACLE_PC_*): foods placed at reset and at respawn, how many of
        each by the forced draw, the most rejections before a valid acceptance; per env since creation or the last clear."""
        out = np.empty((PC_COUNT, self.n), np.int64)
        if lib().salp_oracle_get_placement_counters(self._h, _p(out)) != 0:
            raise RuntimeError("salp_oracle_get_placement_counters failed")
        return out

    def clear_placement_counters(self):
        lib().salp_oracle_clear_placement_counters(self._h)

    def set_placement_limits(self, reset_limit=100, respawn_limit=50):
        """The rejection limits of later resets and respawns (the reference's: 100 and 50).  Guard tests only."""
        if lib().salp_oracle_set_placement_limits(self._h, int(reset_limit), int(respawn_limit)) != 0:
            raise ValueError(f"placement limits ({reset_limit}, {respawn_limit}) out of range")

    def close(self):
        if self._h:
            lib().salp_oracle_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, mask=None):
        obs = np.empty((self.n, self.obs_dim), np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().salp_oracle_reset(self._h, _p(m), _p(obs))
        return obs

    def observe(self):
        obs = np.empty((self.n, self.obs_dim), np.float32)
        lib().salp_oracle_observe(self._h, _p(obs))
        return obs

    def step(self, act, want_final=False):
        act = np.ascontiguousarray(act, dtype=np.float32).reshape(self.n, self.act_dim)
        out = self.rollout(act[None], want_final=want_final)
        return {k: (v[0] if v is not None else None) for k, v in out.items()}

    def rollout(self, act=None, horizon=None, want_final=False, light=False):
        if act is not None:
            act = np.ascontiguousarray(act, dtype=np.float32).reshape(-1, self.n, self.act_dim)
            horizon = act.shape[0]
        H, n = int(horizon), self.n
        if light:  # timing leg: only the last-step outputs are kept by the caller
            obs = reward = r64 = term = trunc = info = None
        else:
            obs = np.empty((H, n, self.obs_dim), np.float32)
            reward = np.empty((H, n), np.float32)
            r64 = np.empty((H, n), np.float64)
            term = np.empty((H, n), np.uint8)
            trunc = np.empty((H, n), np.uint8)
            info = np.empty((H, n, INFO_COLS), np.int32)
        fin = np.full((H, n, self.obs_dim), np.nan, np.float32) if want_final else None
        aout = np.empty((H, n, self.act_dim), np.float32) if (act is None and not light) else None
        rc = lib().salp_oracle_rollout(self._h, _p(act), H, _p(obs), _p(reward), _p(r64), _p(term),
                                       _p(trunc), _p(fin), _p(info), _p(aout))
        if rc != 0:
            raise RuntimeError(f"salp_oracle_rollout failed: {rc}")
        return dict(obs=obs, reward=reward, reward64=r64, terminated=term, truncated=trunc,
                    final_obs=fin, info=info, actions=aout)

    def rollout_f64(self, act64):
        """fp64 actions [H, n, act_dim] (test-only entry point, see oracle/salp_oracle.h)."""
        a = np.ascontiguousarray(act64, dtype=np.float64).reshape(-1, self.n, self.act_dim)
        H = a.shape[0]
        obs = np.empty((H, self.n, self.obs_dim), np.float32)
        r64 = np.empty((H, self.n), np.float64)
        term = np.empty((H, self.n), np.uint8)
        trunc = np.empty((H, self.n), np.uint8)
        rc = lib().salp_oracle_rollout_f64(self._h, _p(a), H, _p(obs), _p(r64), _p(term), _p(trunc))
        if rc != 0:
            raise RuntimeError(f"salp_oracle_rollout_f64 failed: {rc}")
        return dict(obs=obs, reward64=r64, terminated=term, truncated=trunc)

    def get_state(self):
        f64 = np.empty((F_FOOD0 + 2 * self.F, self.n), np.float64)
        i32 = np.empty((I_COUNT, self.n), np.int32)
        lib().salp_oracle_get_state(self._h, _p(f64), _p(i32))
        return f64, i32

    def set_state(self, f64=None, i32=None):
        f = None if f64 is None else np.ascontiguousarray(f64, dtype=np.float64)
        i = None if i32 is None else np.ascontiguousarray(i32, dtype=np.int32)
        lib().salp_oracle_set_state(self._h, _p(f), _p(i))
