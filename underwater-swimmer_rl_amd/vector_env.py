"""Gymnasium-VectorEnv-style host shim over the C ABI (include/salp_vec.h).

`SalpVectorEnv` exposes the surface the reference's consumers use on `SalpSnakeEnv`
(src/salp/environments/salp_snake_env.py:17) for N environments at once:

    reset(seed=None, options=None) -> (obs, info)                       snake:133-155
    step(actions) -> (obs, reward, terminated, truncated, info)         snake:157-202
    num_envs, single_observation_space, single_action_space,
    observation_space, action_space, close()

Observations / rewards / flags are torch tensors resident on the GPU (`output="torch"`, the
default) or numpy arrays (`output="numpy"`, host-pointer ABI).  Autoreset is same-step, as in
gymnasium 0.29's VectorEnv: `info["final_observation"]` holds terminal observations of the
envs flagged in `info["_final_observation"]`.  Attribute pokes of the reference's eval scripts
(`env.robot_pos = ...`, eval/collect_navigation_data.py:76-89) map to `get_state()/set_state()`.

`SalpSB3VecEnv` adapts it to stable-baselines3's `VecEnv` duck type (`step_async/step_wait`,
`dones = terminated | truncated`, `infos[i]["terminal_observation"]`,
`infos[i]["TimeLimit.truncated"]`); `SalpSB3VecEnv.as_sb3_vecenv(...)` makes it a true `VecEnv` subclass where
stable-baselines3 is installed, which is what `SAC("MlpPolicy", env, ...)` (train.py:60-70) checks for
(parity unpinned: SB3 is not importable in the build environment).

PyTorch is used for device buffers and streams only; every simulation call goes through the
C ABI.  If the HIP library or a GPU is missing the constructor raises — there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

from . import _capi
from ._arrays import ArrayBackend, PolicyCache, device_index
from ._capi import SalpLib
from .config import SalpSnakeConfig, load_env_config
from .spaces import batch_space, single_action_space, single_observation_space

ConfigLike = Union[SalpSnakeConfig, str, Dict[str, Any]]


def _as_config(cfg: ConfigLike, **overrides) -> SalpSnakeConfig:
    if isinstance(cfg, SalpSnakeConfig):
        return cfg
    if isinstance(cfg, str):
        return load_env_config(cfg, **overrides)
    return SalpSnakeConfig(**{**cfg, **overrides})


class SalpVectorEnv(ArrayBackend, PolicyCache):
    metadata = {"render_modes": [], "autoreset_mode": "same-step"}
    _handle_class = _capi.PolicyHandle

    def __init__(self, config: ConfigLike = "single_food", num_envs: int = 4096, device: Union[str, int] = "cuda:0",
                 seed: int = 0, env_index_base: int = 0, output: str = "torch", **overrides):
        self.cfg = _as_config(config, **overrides)
        self.num_envs = int(num_envs)
        self.output = output
        if output not in ("torch", "numpy"):
            raise ValueError("output must be 'torch' or 'numpy'")
        self._device_index = device_index(device)
        self.seed_value = int(seed)
        self.env_index_base = int(env_index_base)
        self._lib = SalpLib(self.cfg, self.num_envs, self._device_index, self.seed_value, self.env_index_base)
        self.obs_dim, self.act_dim = self._lib.obs_dim, self._lib.act_dim
        self.single_observation_space = single_observation_space(self.cfg)
        self.single_action_space = single_action_space(self.cfg)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        self.action_space = batch_space(self.single_action_space, self.num_envs)
        self._init_arrays(output, self._device_index)
        self._bufs: Dict[str, Any] = {}
        self._reset_caches()

    def _reset_caches(self):
        self._step_cache = None       # _prepare_step: the step outputs and their raw pointers
        self._packed_cache = {}       # with_final -> the same for step_packed
        self._policy_cache = {}       # id(policy object) -> (policy object, its handle)

    # ------------------------------------------------------------------ buffers
    def _buf(self, name, shape, dtype):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape):
            b = self._bufs[name] = self._empty(shape, dtype)
        return b

    def _out(self, out, key, shape, dtype):
        """The caller's `out[key]` (None included) if it gave one, else the env-owned rollout buffer of that name."""
        return out[key] if out and key in out else self._buf("r_" + key, shape, dtype)

    def _main_outputs(self, out, H, want_obs=True):
        n = self.num_envs
        obs = self._out(out, "obs", (H, n, self.obs_dim), np.float32) if want_obs or (out and "obs" in out) else None
        return (obs, self._out(out, "reward", (H, n), np.float32), self._out(out, "terminated", (H, n), np.uint8),
                self._out(out, "truncated", (H, n), np.uint8))

    def _step_actions(self, actions):
        """(the action block, its address, the current stream) for the direct ctypes call of `step` / `step_packed`: a
        contiguous float32 tensor on this GPU is taken as it is, anything else is converted."""
        t = self._torch
        if t is not None and isinstance(actions, t.Tensor) and actions.is_cuda and actions.device == self.device \
                and actions.dtype == t.float32 and actions.is_contiguous() \
                and actions.numel() == self.num_envs * self.act_dim:
            return actions, actions.data_ptr(), t.cuda.current_stream(self.device).cuda_stream
        a = self._actions_in(actions, (self.num_envs, self.act_dim))
        return a, _capi.address(a), self._stream

    def _rollout_actions(self, actions, horizon):
        """(actions in, the buffer for device-generated actions, H) of an open-loop rollout: one of the first two is None."""
        if actions is not None:
            H = int(actions.shape[0]) if hasattr(actions, "shape") else len(actions)
            return self._actions_in(actions, (H, self.num_envs, self.act_dim)), None, H
        if horizon is None:
            raise ValueError("horizon is required when actions is None")
        H = int(horizon)
        return None, self._buf("r_actions", (H, self.num_envs, self.act_dim), np.float32), H

    def _record_block(self, out, words):
        """The int32 [N, words] block of an evaluation call: `out` (a block, or the dict returned earlier) or a new one."""
        return self._out_block(out["record"] if isinstance(out, dict) else out, (self.num_envs, words), np.int32)

    # ------------------------------------------------------------------ Gymnasium surface
    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None, mask=None):
        """Resets every env (or those in `mask`).  `seed` re-keys the draw streams (the reference's
        reset(seed) only seeds gymnasium's unused np_random, snake:136): `salp_vec_reseed` — new key words, draw counters
        at 0, every env reset, in place.  The C handle, its device state and this env's output buffers are kept (round 2
        destroyed and re-created the handle: a hipGraph captured earlier then replayed into freed memory), so graphs from
        `capture_policy_steps` / `train_sac_graphed` stay valid across `reset(seed=...)`; a poked base_num_food_items
        survives.  A seed restarts EVERY env's stream, so it cannot be combined with a partial `mask`."""
        obs = self._buf("obs", (self.num_envs, self.obs_dim), np.float32)
        if seed is not None:      # any explicit seed restarts the draw streams: reset(seed=s) twice gives the same episodes
            if mask is not None and not bool(np.all(np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask))):
                raise ValueError("reset(seed=..., mask=...) with a partial mask: a seed re-keys the draw streams of ALL envs; "
                                 "reseed with mask=None, or reset the subset without a seed")
            self.seed_value = int(seed)
            self._lib.reseed(self.seed_value, obs, self._flags, self._stream)
        else:
            self._lib.reset(self._mask_in(mask), obs, self._flags, self._stream)
        return obs, {}

    def _prepare_step(self):
        """Allocates the step outputs once and caches their raw pointers (the per-call cost of
        `step` is then one ctypes call: at H = 1 the host, not the kernel, is the bottleneck)."""
        n = self.num_envs
        obs = self._buf("obs", (n, self.obs_dim), np.float32)
        rew = self._buf("reward", (n,), np.float32)
        term = self._buf("terminated", (n,), np.uint8)
        trunc = self._buf("truncated", (n,), np.uint8)
        info_i = self._buf("info", (n, _capi.INFO_COLS), np.int32)
        fin = self._buf("final_obs", (n, self.obs_dim), np.float32)
        done = self._empty((n,), np.bool_)
        info = {"food_collected": info_i[:, 0], "steps_since_food": info_i[:, 1], "collision": info_i[:, 2],
                "final_observation": fin, "_final_observation": done}
        ptr = lambda x: ctypes.c_void_p(_capi.address(x))
        self._step_cache = dict(obs=obs, rew=rew, term=self._bool_view(term), trunc=self._bool_view(trunc), info=info, done=done,
                                p_obs=ptr(obs), p_rew=ptr(rew), p_term=ptr(term), p_trunc=ptr(trunc),
                                p_fin=ptr(fin), p_info=ptr(info_i), fn=self._lib.lib.salp_vec_step, h=self._lib._h,
                                flags=self._flags, logical_or=(self._torch or np).logical_or)
        return self._step_cache

    def step(self, actions, want_final_observation: bool = True):
        """One step of every env.  The returned tensors are the env's own output buffers: they are
        overwritten by the next call (clone what must be kept).  `info["score"]` of the reference
        (snake:196) is `info["food_collected"] * food_reward`."""
        c = self._step_cache or self._prepare_step()
        a, p_act, stream = self._step_actions(actions)
        rc = c["fn"](c["h"], p_act, c["p_obs"], c["p_rew"], c["p_term"], c["p_trunc"],
                     c["p_fin"] if want_final_observation else None, c["p_info"], c["flags"], stream)
        if rc != 0:
            _capi.check(self._lib.lib, rc, "salp_vec_step")
        if want_final_observation:
            c["logical_or"](c["term"], c["trunc"], out=c["done"])
        return c["obs"], c["rew"], c["term"], c["trunc"], c["info"]

    def _prepare_step_packed(self, with_final: bool):
        rec = self._buf("rec_final" if with_final else "rec", (self.num_envs, self._lib.record_width(with_final)), np.float32)
        c = self._packed_cache[with_final] = dict(
            rec=rec, p_rec=ctypes.c_void_p(_capi.address(rec)), fn=self._lib.lib.salp_vec_step_packed, h=self._lib._h,
            flags=self._flags | (_capi.REC_FINAL_OBS if with_final else 0))
        return c

    def step_packed(self, actions, want_final_observation: bool = True):
        """One step of every env, returned as ONE block: the packed transition records [N, width] (records.py;
        `unpack_record(rec, obs_dim)` gives the step tuple's fields as zero-copy views).  width = obs_dim + 4, or
        2 obs_dim + 4 with terminal observations (the tail of an unfinished env's row is not written).  The block is the
        env's own buffer, overwritten by the next call; the per-call cost is one ctypes call, as in `step`."""
        with_final = bool(want_final_observation)
        c = self._packed_cache.get(with_final) or self._prepare_step_packed(with_final)
        a, p_act, stream = self._step_actions(actions)
        rc = c["fn"](c["h"], p_act, c["p_rec"], c["flags"], stream)
        if rc != 0:
            _capi.check(self._lib.lib, rc, "salp_vec_step_packed")
        return c["rec"]

    def rollout_packed(self, actions=None, horizon: Optional[int] = None, want_final_observation: bool = False,
                       out=None) -> dict:
        """`horizon` steps in one kernel launch with the packed records as the only output: dict(record=[H, N, width],
        actions=...).  actions: [H, N, act_dim] or None (device-generated).  `out`: a float32 [H, N, width] block to write
        into (its width must match `want_final_observation`); default an env-owned buffer."""
        a, aout, H = self._rollout_actions(actions, horizon)
        with_final = bool(want_final_observation)
        shape = (H, self.num_envs, self._lib.record_width(with_final))
        rec = out if out is not None else self._buf("r_rec_final" if with_final else "r_rec", shape, np.float32)
        if tuple(rec.shape) != shape:
            raise ValueError(f"out has shape {tuple(rec.shape)}; expected {shape}")
        self._lib.rollout_packed(a, H, rec, aout, self._flags | (_capi.REC_FINAL_OBS if with_final else 0), self._stream)
        return dict(record=rec, actions=a if a is not None else aout)

    def capture_policy_steps(self, policy, n_steps: int = 1, record=None, want_final_observation: bool = True):
        """Captures `n_steps` x (`policy(obs) -> actions`, `step(actions)`) into one hipGraph and returns the
        `torch.cuda.CUDAGraph`; every `replay()` advances all envs by `n_steps`.  For small batches the
        acting loop is launch-bound (one step kernel runs in a few microseconds), and a replay costs one
        host call whatever `n_steps` is.  `record(k, obs, actions, reward, terminated, truncated, info)`,
        if given, is called inside the capture after step k (e.g. to copy the transition into
        preallocated replay storage with torch ops); `obs` is the observation the policy saw (a clone).
        The body runs once un-captured as a warm-up (so does `record`); the env state is restored after it.
        `salp_vec_step` with device pointers is only kernel launches on the caller's stream, so it is
        capturable; device-generated actions (`rollout(actions=None)`) are not, their step index lives
        on the host.  After a replay the env's step outputs (`step`'s return buffers) hold the last step."""
        t = self._torch
        if t is None:
            raise _capi.SalpError("capture_policy_steps needs output='torch'")
        obs = (self._step_cache or self._prepare_step())["obs"]

        def body():
            for k in range(int(n_steps)):
                seen = obs.clone() if record is not None else obs
                a = policy(seen).to(t.float32).reshape(self.num_envs, self.act_dim).contiguous()
                o, r, te, tr, info = self.step(a, want_final_observation=want_final_observation)
                if record is not None:
                    record(k, seen, a, r, te, tr, info)

        # warm-up on a side stream (allocator pools, lazy kernel loads), then restore the envs
        f64, i32 = self.get_state()
        obs0 = obs.clone()
        side = t.cuda.Stream(device=self.device)
        side.wait_stream(t.cuda.current_stream(self.device))
        with t.cuda.stream(side):
            body()
        t.cuda.current_stream(self.device).wait_stream(side)
        t.cuda.synchronize(self.device)
        self.set_state(f64, i32)
        obs.copy_(obs0)
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g):
            body()
        # capture does not execute: state and obs are still those of before the call
        return g

    def rollout(self, actions=None, horizon: Optional[int] = None, want_obs: bool = True,
                want_final_observation: bool = False, out: Optional[dict] = None) -> dict:
        """`horizon` steps in one kernel launch.  actions: [H, N, act_dim] or None (device-generated)."""
        a, aout, H = self._rollout_actions(actions, horizon)
        obs, rew, term, trunc = self._main_outputs(out, H, want_obs)
        fin = self._buf("r_final", (H, self.num_envs, self.obs_dim), np.float32) if want_final_observation else None
        self._lib.rollout(a, H, obs, rew, term, trunc, fin, aout, self._flags, self._stream)
        return dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_obs=fin,
                    actions=a if a is not None else aout)

    def make_policy(self, policy, weights=None):
        """An in-kernel policy of this env (`policy.MLPPolicy` or `policy.GaussianPolicy`, one policy or a population): a
        `_capi.PolicyHandle` for `rollout_policy` (a Gaussian one also for `sample=True`; it carries `noise_step`).  `handle.update(w, flags, stream)` takes new weights of the same shape in the public layout
        (`MLPPolicy.pack()`); with a device tensor and SALP_DEVICE_PTRS it is stream-ordered and allocates nothing."""
        self._check_policy(policy)
        return self._lib.policy_create(policy, weights, 0 if weights is None else self._flags, self._stream)

    def rollout_policy(self, policy, horizon: int, want_actions: bool = True, out: Optional[dict] = None, sample: bool = False) -> dict:
        """`horizon` closed-loop steps in one kernel launch: every action is `policy` applied to the observation before it
        (the first one to the current observation).  `policy`: a handle of `make_policy`, or an `MLPPolicy` (a handle is
        then made and kept for the next call with the same object).  Returns the dict of `rollout` with `actions`
        ([H, N, act_dim], None without `want_actions`).  `sample=True` (a `GaussianPolicy`): the actions are sampled in
        the kernel (tanh-Gaussian, the policy's noise stream) and the dict gains `logp` [H, N]; with `sample=False` a
        Gaussian policy runs its mean."""
        policy = self._policy_handle(policy)
        H, n = int(horizon), self.num_envs
        if H < 1:
            raise ValueError("horizon must be >= 1")
        obs, rew, term, trunc = self._main_outputs(out, H)
        aout = self._out(out, "actions", (H, n, self.act_dim), np.float32) if want_actions else None
        if sample:
            logp = self._out(out, "logp", (H, n), np.float32)
            self._lib.rollout_policy_sampled(policy, H, obs, rew, term, trunc, aout, logp, self._flags, self._stream)
            return dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_obs=None, actions=aout, logp=logp)
        self._lib.rollout_policy(policy, H, obs, rew, term, trunc, aout, self._flags, self._stream)
        return dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_obs=None, actions=aout)

    def rollout_policy_packed(self, policy, horizon: int, want_final_observation: bool = True, want_actions: bool = True,
                              sample: bool = False, out=None) -> dict:
        """The closed loop of `rollout_policy` with the packed records of `rollout_packed` as its output
        (salp_vec_rollout_policy_packed): dict(record=[H, N, width], actions=[H, N, act_dim] or None) and, with
        `sample=True` (a `GaussianPolicy`), `logp` [H, N].  The record keeps what `rollout_policy` cannot return: the info
        counters, the collision byte and — with `want_final_observation` — the terminal observation of every finished row
        (`records.unpack_record` gives the views, `records.transitions` the replay tuples over all H x N rows).  `out`: a
        float32 [H, N, width] block to write into (its width must match `want_final_observation`); default an env-owned
        buffer."""
        policy = self._policy_handle(policy)
        H, n = int(horizon), self.num_envs
        if H < 1:
            raise ValueError("horizon must be >= 1")
        with_final = bool(want_final_observation)
        shape = (H, n, self._lib.record_width(with_final))
        rec = out if out is not None else self._buf("r_rec_final" if with_final else "r_rec", shape, np.float32)
        if tuple(rec.shape) != shape:
            raise ValueError(f"out has shape {tuple(rec.shape)}; expected {shape}")
        aout = self._buf("r_actions", (H, n, self.act_dim), np.float32) if want_actions else None
        flags = self._flags | (_capi.REC_FINAL_OBS if with_final else 0)
        if sample:
            logp = self._buf("r_logp", (H, n), np.float32)
            self._lib.rollout_policy_packed_sampled(policy, H, rec, aout, logp, flags, self._stream)
            return dict(record=rec, actions=aout, logp=logp)
        self._lib.rollout_policy_packed(policy, H, rec, aout, flags, self._stream)
        return dict(record=rec, actions=aout)

    def evaluate_policy(self, policy, horizon: int, out=None, accumulate: bool = False, sample: bool = False) -> dict:
        """`horizon` closed-loop steps of `rollout_policy` in one kernel launch with NO per-step output: one summary record
        per env (32 B) instead of [H, N] observations, rewards and flags.  Returns typed views of one int32 [N, 8] block
        (`policy.evaluation_views`): `record`, `return_sum` and `first_return` (float64 [N]: the float32 step rewards added
        in step order — over the call, and up to the env's first episode end), `first_length`, `first_end` (0 not finished,
        1 terminated, 2 truncated), `episodes`, `food` (int32 [N]).  `out`: a block (or a dict returned earlier) to write
        into; `accumulate=True` continues the records in `out` (required then), so that a run cut into several calls gives
        the bits of one call.  A policy's score: `return_sum.view(P, E).mean(1)`.  `sample=True` (a `GaussianPolicy`):
        the run takes the policy's sampled actions, as `rollout_policy(..., sample=True)` would."""
        from .policy import EVAL_WORDS, evaluation_views
        policy = self._policy_handle(policy)
        H = int(horizon)
        if H < 1:
            raise ValueError("horizon must be >= 1")
        if accumulate and out is None:
            raise ValueError("accumulate=True continues the records in `out`: pass the block of the call before")
        rec = self._record_block(out, EVAL_WORDS)
        views = evaluation_views(rec)       # checks dtype and contiguity
        call = self._lib.evaluate_policy_sampled if sample else self._lib.evaluate_policy
        call(policy, H, rec, self._flags | (_capi.EVAL_ACCUMULATE if accumulate else 0), self._stream)
        return views

    def evaluate_navigation(self, policy, horizon: int, line, goal_radius: float = 50.0, out=None, accumulate: bool = False,
                            track: bool = False) -> dict:
        """Fixed start -> goal trials in one kernel launch (salp_vec_evaluate_navigation): up to `horizon` closed-loop steps
        of `rollout_policy`, every env stopping — not stepped any further — once it is within `goal_radius` of its goal.
        `line`: [4] or [N, 4] float64 (start x, start y, goal x, goal y); the envs are expected at their starts
        (`set_state`).  Needs one food, forced breathing and `no_autoreset` (`navigation_eval.navigation_config`).  Returns
        typed views of one int32 [N, 20] block (`policy.navigation_views`): `record`, `steps`, `status` (bit 0 reached, bit 1
        collided, bit 2 captured the food), `path_sum`, `lateral_sum`, `xmin`, `xmax`, `ymin`, `ymax`, `x`, `y` (float64
        [N]) — and with `track=True` also `track`, float64 [horizon, N, 2]: the position after each step of this call, a
        stopped env repeating its last one (`track` may also be the block to write into).  `out` / `accumulate` as in `evaluate_policy`: a run cut into several calls
        gives the bits of one call."""
        from .policy import NAV_WORDS, navigation_line, navigation_views
        H, n = int(horizon), self.num_envs
        if H < 1:
            raise ValueError("horizon must be >= 1")
        radius = float(goal_radius)
        if not (np.isfinite(radius) and radius > 0.0):
            raise ValueError("goal_radius must be finite and positive")
        if accumulate and out is None:
            raise ValueError("accumulate=True continues the records in `out`: pass the block of the call before")
        t = self._torch
        # a float64 [N, 4] tensor on this GPU is taken as it is (nothing is copied or allocated for it: capturable)
        on_device = t is not None and isinstance(line, t.Tensor) and line.device == self.device
        if on_device:
            if not self._is_block(line, (n, 4), np.float64):
                raise ValueError(f"a device line must be a contiguous float64 [{n}, 4] tensor")
            ln = line
        else:
            ln = navigation_line(line.cpu().numpy() if t is not None and isinstance(line, t.Tensor) else line, n)
        cfg = self.cfg
        if cfg.num_food_items != 1 or not cfg.forced_breathing or not cfg.no_autoreset or cfg.max_observed_food != 3:
            raise ValueError("evaluate_navigation needs num_food_items == 1, forced breathing, max_observed_food == 3 and no_autoreset")
        policy = self._policy_handle(policy)
        rec = self._record_block(out, NAV_WORDS)
        views = navigation_views(rec)       # checks dtype and contiguity
        want_track = track is not None and track is not False
        given = want_track and track is not True       # a block to write into: float64 [H, N, 2], on this GPU for a torch env
        if t is not None and not on_device:
            ln = t.from_numpy(ln).to(self.device)
        if given and not self._is_block(track, (H, n, 2), np.float64):
            raise ValueError(f"a track block must be a contiguous float64 [{H}, {n}, 2] " +
                             ("array" if t is None else f"tensor on {self.device}"))
        trk = track if given else (self._empty((H, n, 2), np.float64) if want_track else None)
        self._lib.evaluate_navigation(policy, H, ln, radius, rec, trk, self._flags | (_capi.EVAL_ACCUMULATE if accumulate else 0),
                                      self._stream)
        if want_track:
            views["track"] = trk
        return views

    def observe(self):
        obs = self._buf("obs", (self.num_envs, self.obs_dim), np.float32)
        self._lib.observe(obs, self._flags, self._stream)
        return obs

    def close(self):
        self._lib.close()
        self._bufs.clear()
        self._reset_caches()

    # ------------------------------------------------------------------ state access
    def get_state(self):
        """(f64 [SALP_F_COUNT(F), N], i32 [SALP_I_COUNT, N]) host numpy arrays; rows in _capi.F_* / I_*."""
        F = self.cfg.num_food_items
        f64 = np.empty((_capi.F_FOOD0 + 2 * F, self.num_envs), np.float64)
        i32 = np.empty((_capi.I_COUNT, self.num_envs), np.int32)
        if self._torch is not None:
            self._torch.cuda.current_stream(self.device).synchronize()
        self._lib.get_state(f64, i32, 0, 0)
        return f64, i32

    def set_state(self, f64=None, i32=None):
        f = None if f64 is None else np.ascontiguousarray(f64, dtype=np.float64)
        i = None if i32 is None else np.ascontiguousarray(i32, dtype=np.int32)
        if self._torch is not None:
            self._torch.cuda.current_stream(self.device).synchronize()
        self._lib.set_state(f, i, 0, 0)

    # the attributes the reference's callers read/poke, as whole-batch arrays
    @property
    def robot_pos(self):
        f, _ = self.get_state()
        return np.stack([f[_capi.F_X], f[_capi.F_Y]], axis=1)

    @property
    def robot_velocity(self):
        f, _ = self.get_state()
        return np.stack([f[_capi.F_VX], f[_capi.F_VY]], axis=1)

    @property
    def robot_angle(self):
        return self.get_state()[0][_capi.F_THETA]

    @property
    def food_positions(self):
        f, _ = self.get_state()
        F = self.cfg.num_food_items
        return np.stack([f[_capi.F_FOOD0:_capi.F_FOOD0 + F].T, f[_capi.F_FOOD0 + F:_capi.F_FOOD0 + 2 * F].T], axis=2)

    @property
    def num_food_items(self):
        """Per env, the number of foods of its CURRENT episode (what continuous_trainer.py:380 reads from the single
        env: `base_num_food_items`, or the episode's draw with random_food_count).  Recovered from the state: live
        foods, plus the captured ones when foods do not respawn."""
        f64, i32 = self.get_state()
        F = self.cfg.num_food_items
        live = (~np.isnan(f64[_capi.F_FOOD0:_capi.F_FOOD0 + F])).sum(axis=0)
        return live if self.cfg.respawn_food else live + i32[_capi.I_FOOD_COLLECTED]

    @property
    def base_num_food_items(self) -> int:
        """The attribute the reference's curriculum writes (continuous_trainer.py:409-411; snake:36): foods
        placed at every later reset, 0..cfg.num_food_items (the slots the env was created with)."""
        return self._lib.base_num_food

    @base_num_food_items.setter
    def base_num_food_items(self, k: int):
        self._lib.set_base_num_food(k)

    def stats(self) -> dict:
        return self._lib.stats()

    def clear_stats(self):
        self._lib.clear_stats()

    @property
    def global_step(self) -> int:
        return self._lib.global_step


class _LazyInfos(Sequence):
    """SB3 wants `list[dict]` per step; at thousands of envs that list is the bottleneck, so the
    dicts are materialised on access."""

    def __init__(self, n, food, ssf, coll, dones, truncs, terminal_obs, food_reward):
        self._n, self._food, self._ssf, self._coll = n, food, ssf, coll
        self._dones, self._truncs, self._tobs, self._fr = dones, truncs, terminal_obs, food_reward

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        d = {"food_collected": int(self._food[i]), "steps_since_food": int(self._ssf[i]),
             "collision": bool(self._coll[i]), "score": float(self._food[i]) * self._fr,
             "TimeLimit.truncated": bool(self._truncs[i])}
        if self._dones[i]:
            d["terminal_observation"] = self._tobs[i]
        return d


class SalpSB3VecEnv:
    """The method surface of stable-baselines3's `VecEnv` over SalpVectorEnv (numpy in / numpy out): `reset`,
    `step_async` / `step_wait`, `dones = terminated | truncated`, `infos[i]["terminal_observation"]`,
    `"TimeLimit.truncated"`, `get_attr / set_attr / env_method / env_is_wrapped`.  It is a duck type, NOT a subclass:
    stable-baselines3 is not installable in the build environment, so whether `SAC("MlpPolicy", env)` accepts it as
    is — SB3's `_wrap_env` tests `isinstance(env, VecEnv)` — is parity unpinned; `as_sb3_vecenv()` returns an
    instance of a real `VecEnv` subclass when stable-baselines3 is importable."""

    @classmethod
    def as_sb3_vecenv(cls, *args, **kwargs):
        """With stable-baselines3 importable: an instance of a class deriving from BOTH this adapter and SB3's
        `VecEnv` (so `isinstance(env, VecEnv)` holds and SB3 does not wrap it in a DummyVecEnv); raises
        ImportError otherwise."""
        from stable_baselines3.common.vec_env import VecEnv      # ImportError where SB3 is absent
        sub = type("SalpSB3VecEnvSubclass", (cls, VecEnv), {})
        self = sub.__new__(sub)
        cls.__init__(self, *args, **kwargs)
        VecEnv.__init__(self, self.num_envs, self.observation_space, self.action_space)
        return self

    def __init__(self, config: ConfigLike = "single_food", num_envs: int = 8, device: Union[str, int] = 0,
                 seed: int = 0, **overrides):
        self.venv = SalpVectorEnv(config, num_envs, device=device, seed=seed, output="numpy", **overrides)
        self.num_envs = self.venv.num_envs
        self.observation_space = self.venv.single_observation_space
        self.action_space = self.venv.single_action_space
        self.render_mode = None
        self._actions = None

    def reset(self):
        obs, _ = self.venv.reset()
        return obs.copy()

    def step_async(self, actions):
        self._actions = np.asarray(actions, dtype=np.float32)

    def step_wait(self):
        obs, rew, term, trunc, info = self.venv.step(self._actions)
        dones = term | trunc
        infos = _LazyInfos(self.num_envs, info["food_collected"].copy(), info["steps_since_food"].copy(),
                           info["collision"].copy(), dones, trunc & ~term, info["final_observation"].copy(),
                           float(self.venv.cfg.food_reward))
        return obs.copy(), rew.copy(), dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.venv.close()

    def seed(self, seed=None):
        if seed is not None:
            self.venv.reset(seed=seed)
        return [seed] * self.num_envs

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        if isinstance(indices, int):
            return [indices]
        return indices

    def get_attr(self, attr_name, indices=None):
        idx = list(self._indices(indices))
        if hasattr(self.venv.cfg, attr_name):
            return [getattr(self.venv.cfg, attr_name)] * len(idx)
        v = getattr(self.venv, attr_name)
        if np.ndim(v) == 0:
            return [v] * len(idx)
        return [v[i] for i in idx]

    def set_attr(self, attr_name, value, indices=None):
        if attr_name == "base_num_food_items":      # the one parameter the reference's trainers poke
            self.venv.base_num_food_items = value
            return
        raise AttributeError(f"{attr_name}: parameters are fixed at construction; state goes through set_state()")

    def env_method(self, method_name, *args, indices=None, **kwargs):
        raise AttributeError(f"env_method({method_name}) is not supported by the batched simulator")

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(list(self._indices(indices)))

    def get_images(self):
        return [None] * self.num_envs

    def render(self, mode=None):
        return None
