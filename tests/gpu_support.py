"""Helpers shared by the GPU test files: handles put into a start state, output blocks, and the comparisons with the
project's tolerances (north_star: "within 1e-5 fp32"):
  * terminated / truncated / info integers: identical;
  * observation: max |diff| <= 1e-5 (support.obs_diff: angle columns on the circle, NaN fails);
  * reward: |diff| <= 1e-5 * max(1, |reward|);
  * fp64 state snapshot: |diff| <= 1e-9 (only device sin/cos and d^2-vs-sqrt predicates differ)."""
import numpy as np

import parity_cases as pc
from support import obs_diff
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpLib

OBS_TOL = 1e-5
REW_TOL = 1e-5
STATE_TOL = 1e-9


def device_state(dev, cfg):
    f64 = np.empty((_capi.F_FOOD0 + 2 * cfg.num_food_items, dev.n_envs), np.float64)
    i32 = np.empty((_capi.I_COUNT, dev.n_envs), np.int32)
    dev.get_state(f64, i32, 0)
    return f64, i32


def started(cfg, n, f64, i32, seed=pc.ENV_SEED, base=0):
    """A handle whose envs have the global indices base .. base + n - 1, put into the start state (f64, i32)."""
    dev = SalpLib(cfg, n, device_id=0, seed=seed, env_index_base=base)
    dev.set_state(f64, i32, 0)
    return dev


def start_pair(cfg, n, seed, **kw):
    """Device and oracle in the shared injected start state (tests/parity_cases.py), set through set_state on both."""
    orc, f64, i32 = pc.start_oracle(cfg, n, seed, **kw)
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    dev.set_state(f64, i32, 0)
    return dev, orc


def run_device(cfg, n, act=None, horizon=None, seed=0, base=0, want_final=False, dev=None):
    own = dev is None
    if own:
        dev = SalpLib(cfg, n, device_id=0, seed=seed, env_index_base=base)
    H = act.shape[0] if act is not None else horizon
    obs = np.empty((H, n, cfg.obs_dim), np.float32)
    rew = np.empty((H, n), np.float32)
    term = np.empty((H, n), np.uint8)
    trunc = np.empty((H, n), np.uint8)
    fin = np.full((H, n, cfg.obs_dim), np.nan, np.float32) if want_final else None
    aout = np.empty((H, n, cfg.act_dim), np.float32) if act is None else None
    dev.rollout(act, H, obs, rew, term, trunc, fin, aout, 0)
    out = dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_obs=fin, actions=aout)
    return (out, dev) if not own else (out, dev)


def host_outputs(cfg, horizon, n, logp=False):
    """Host output blocks that no kernel output can be mistaken for: NaN floats, flag bytes of 7."""
    o = dict(obs=np.full((horizon, n, cfg.obs_dim), np.nan, np.float32), reward=np.full((horizon, n), np.nan, np.float32),
             terminated=np.full((horizon, n), 7, np.uint8), truncated=np.full((horizon, n), 7, np.uint8),
             actions=np.full((horizon, n, cfg.act_dim), np.nan, np.float32))
    if logp:
        o["logp"] = np.full((horizon, n), np.nan, np.float32)
    return o


def run_policy(dev, ph, cfg, horizon, want_actions=True):
    o = host_outputs(cfg, horizon, dev.n_envs)
    dev.rollout_policy(ph, horizon, o["obs"], o["reward"], o["terminated"], o["truncated"], o["actions"] if want_actions else None, 0)
    return o


def run_sampled(dev, ph, cfg, horizon, want_actions=True, want_logp=True):
    o = host_outputs(cfg, horizon, dev.n_envs, logp=True)
    dev.rollout_policy_sampled(ph, horizon, o["obs"], o["reward"], o["terminated"], o["truncated"],
                               o["actions"] if want_actions else None, o["logp"] if want_logp else None, 0)
    return o


def assert_parity(cfg, got, ref, label=""):
    assert np.array_equal(got["terminated"], ref["terminated"]), f"{label}: terminated flags differ"
    assert np.array_equal(got["truncated"], ref["truncated"]), f"{label}: truncated flags differ"
    d = obs_diff(cfg, got["obs"], ref["obs"])
    assert d.max() <= OBS_TOL, f"{label}: obs diff {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    rd = np.abs(got["reward"].astype(np.float64) - ref["reward64"]) / np.maximum(1.0, np.abs(ref["reward64"]))
    assert rd.max() <= REW_TOL, f"{label}: reward diff {rd.max()}"
    return float(d.max()), float(rd.max())


def assert_state_parity(cfg, dev, state_or_oracle, label=""):
    """The device's state against an (f64, i32) snapshot, or against an oracle's own get_state()."""
    f_d, i_d = device_state(dev, cfg)
    f_o, i_o = state_or_oracle.get_state() if hasattr(state_or_oracle, "get_state") else state_or_oracle
    assert np.array_equal(i_d, i_o), f"{label}: integer state differs in rows {np.unique(np.nonzero(i_d != i_o)[0])}"
    both_nan = np.isnan(f_d) & np.isnan(f_o)
    assert np.array_equal(np.isnan(f_d), np.isnan(f_o)), f"{label}: food None-pattern differs"
    d = np.where(both_nan, 0.0, np.abs(f_d - f_o))
    assert d.max() <= STATE_TOL, f"{label}: fp64 state diff {d.max()} in row {np.unravel_index(d.argmax(), d.shape)}"


def assert_final_obs(cfg, got_fin, ref, label=""):
    """Terminal observations are delivered for finished envs, and only for them, with the oracle's values."""
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert done.any(), f"{label}: no episode ends: the terminal branch is not tested"
    assert np.array_equal(np.isnan(got_fin[..., 0]), ~done), f"{label}: final_obs rows written do not match the finished envs"
    d = obs_diff(cfg, got_fin[done], ref["final_obs"][done])
    assert d.max() <= OBS_TOL, f"{label}: final_obs diff {d.max()}"
    return float(d.max())
