"""Batched HEAD simulator: the reference's `SalpRobotEnv(robot=Robot(...))`
(src/salp/environments/salp_robot_env.py over robot.py) for N robots on one MI355X.

    env = SalpRobotVectorEnv(num_envs=65536, device="cuda:0", seed=0)
    obs, _ = env.reset()
    obs, reward, terminated, truncated, info = env.step(actions)      # actions [N, 3] in [0,1]x[0,1]x[-1,1]

One `step` is one whole breathing cycle of every robot (Robot.set_control + step_through_cycle,
robot.py:335-358, 422-445): `info["inner_steps"]` is the number of Euler steps each robot took.
`env.record_history(slice(a, b), stride)` adds the per-Euler-step history of those robots to `info`
(`cycle_history`, `cycle_history_len`, `cycle_history_envs`; `env.history_of(i)` in the reference's shape).
`env.rollout(actions_HN3)` runs H cycles of every robot in one launch, and `env.rollout_policy(policy, H)` does so with
every action computed in the kernel by a small MLP policy (`policy.MLPPolicy`, 6 observations -> 3 action components);
with a `policy.GaussianPolicy` and `sample=True` the kernel samples the tanh-Gaussian action and returns its log-probability.
`env.evaluate_policy(policy, H)` is that closed loop with no per-step output: one summary record per robot, continuable
across calls (`accumulate=True`) and, with `first_episode=True`, stopped at the end of each robot's first episode.
Same conventions as SalpVectorEnv: device tensors, same-step autoreset with `final_observation`,
no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _capi
from ._arrays import ArrayBackend, PolicyCache, device_index
from ._capi import ROBOT_EXPORTS, CRobotConfig  # noqa: F401  (imported from here by tests and robot_compare.py)
from .spaces import Box, batch_space

(R_POS, R_VEL, R_EULER, R_OMEGA, R_VEL_WORLD, R_PREV_I, R_TARGET, R_PREV_DIST, R_VOLUME, R_ANGLE1, R_ANGLE2, R_TIME,
 R_CYCLE, R_RNG, R_COUNT) = 0, 3, 6, 9, 12, 15, 18, 20, 21, 22, 23, 24, 25, 26, 27

# channels of one cycle-history sample (SALP_H_* of include/salp_robot.h)
(H_POS, H_VEL, H_EULER, H_OMEGA, H_LENGTH, H_WIDTH, H_STATE, H_NOZZLE_YAW, H_COUNT) = 0, 3, 6, 9, 12, 13, 14, 15, 16
# history_of(i) keys (the reference's Robot.*_history names) -> (first channel, width; None = scalar per sample)
HISTORY_CHANNELS = {"position_history": (H_POS, 3), "velocity_history": (H_VEL, 3), "euler_angle_history": (H_EULER, 3),
                    "angular_velocity_history": (H_OMEGA, 3), "length_history": (H_LENGTH, None),
                    "width_history": (H_WIDTH, None), "state_history": (H_STATE, None),
                    "nozzle_yaw_history": (H_NOZZLE_YAW, None)}


class RobotPolicyHandle(_capi.PolicyHandleBase):
    """One salp_robot_policy_t (SalpRobotVectorEnv.make_policy); `env` made it."""
    _prefix = "salp_robot_policy_"
    _what = {"noise_step": "noise_step", "set_noise_step": "set_noise_step", "update": "policy update"}
    env = property(lambda self: self.owner)

    def set_noise_step(self, n: int, stream=None):
        """salp_robot_policy_set_noise_step: stream-ordered on `stream` (default: the env's current one)."""
        super().set_noise_step(n, self.env._stream if stream is None else stream)

    def update(self, weights, flags=None, stream=None):
        """salp_robot_policy_update: float32 [P, words] in the public layout — a numpy array (flags 0), or a device tensor
        (SALP_DEVICE_PTRS: stream-ordered on `stream`, default the current one, no allocation)."""
        if flags is None:
            flags = _capi.SALP_DEVICE_PTRS if hasattr(weights, "data_ptr") else 0
        super().update(weights, flags, self.env._stream if stream is None else stream)


class SalpRobotVectorEnv(ArrayBackend, PolicyCache):
    _handle_class = RobotPolicyHandle

    def __init__(self, num_envs: int = 4096, device="cuda:0", seed: int = 0, env_index_base: int = 0,
                 output: str = "torch", **robot_params):
        self.L = self.lib = _capi.load_library()     # `lib`: the name a policy handle asks its owner for, as SalpLib has it
        self.num_envs = int(num_envs)
        cfg = CRobotConfig()
        _capi.call(self.L, "salp_robot_config_default", ctypes.byref(cfg))
        for k, v in robot_params.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown robot parameter {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self._device_index = device_index(device)
        self._h = ctypes.c_void_p()
        _capi.call(self.L, "salp_robot_vec_create", ctypes.byref(cfg), self.num_envs, self._device_index, int(seed),
                   int(env_index_base), ctypes.byref(self._h))
        self.obs_dim, self.act_dim = 6, 3
        # salp_robot_env.py:48-69
        self.single_action_space = Box(low=np.array([0.0, 0.0, -1.0]), high=np.array([1.0, 1.0, 1.0]), dtype=np.float32)
        self.single_observation_space = Box(low=np.full(6, -np.inf), high=np.full(6, np.inf), dtype=np.float32)
        self.action_space = batch_space(self.single_action_space, self.num_envs)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        self._init_arrays(output, self._device_index)
        n = self.num_envs
        self._obs, self._fin = self._empty((n, 6), np.float32), self._empty((n, 6), np.float32)
        self._rew, self._term, self._trunc = self._empty((n,), np.float32), self._empty((n,), np.uint8), self._empty((n,), np.uint8)
        self._inner = self._empty((n,), np.int32)
        self._hist = None      # (begin, count, stride, capacity, history, history_len) while record_history is on
        self._bufs = {}        # rollout outputs by name, cached per H
        self._policies = []    # RobotPolicyHandle objects made on this env
        self._policy_cache = {}   # id(policy object) -> (policy object, its handle)

    _p = staticmethod(_capi.address)

    def _call(self, name, *args, what):
        _capi.call(self.L, name, self._h, *args, self._flags, self._stream, what=what)

    def reset(self, *, seed: Optional[int] = None, options=None, mask=None):
        self._call("salp_robot_vec_reset", self._mask_in(mask), self._obs, what="reset")
        return self._obs, {}

    def observe(self):
        zero = self._empty((self.num_envs,), np.uint8)
        zero[...] = 0
        self._call("salp_robot_vec_reset", zero, self._obs, what="observe")
        return self._obs

    def history_capacity(self, stride: int = 1) -> int:
        """Most samples one cycle can record per env at this stride (salp_robot_vec_history_capacity)."""
        c = self.L.salp_robot_vec_history_capacity(self._h, int(stride))
        if c < 0:
            raise ValueError(f"no history at stride {stride}: stride must be >= 1 and a cycle at most 2^24 Euler steps")
        return int(c)

    def record_history(self, envs=None, stride: int = 1):
        """Records the per-Euler-step history of every later `step` for the envs `envs` (a slice with step 1, None for
        all of them) every `stride` Euler steps; `record_history(False)` turns recording off.  The buffers are allocated
        here and reused by every step: `info["cycle_history"]` float32 [R, capacity, 16] (channels H_*, samples past
        `info["cycle_history_len"]` int32 [R] unspecified), `info["cycle_history_envs"]` = (begin, R)."""
        if envs is False:
            self._hist = None
            return
        if envs is None or envs is True:
            envs = slice(0, self.num_envs)
        if not isinstance(envs, slice) or envs.step not in (None, 1):
            raise TypeError("envs must be a contiguous slice(a, b), None or False")
        begin, end, _ = envs.indices(self.num_envs)
        count = max(0, end - begin)
        if count == 0:
            raise ValueError(f"empty env range {envs}")
        cap = self.history_capacity(stride)
        self._hist = (begin, count, int(stride), cap, self._empty((count, cap, H_COUNT), np.float32), self._empty((count,), np.int32))

    def history_of(self, i: int) -> dict:
        """The reference-shaped cycle history (Robot.*_history after step_through_cycle) of recorded env `i` for the
        last step: float64 numpy arrays of length L = its sample count ([L, 3] for vectors), `state_history` int."""
        if self._hist is None:
            raise RuntimeError("record_history is off")
        begin, count = self._hist[0], self._hist[1]
        if not begin <= i < begin + count:
            raise IndexError(f"env {i} is not recorded (recorded: [{begin}, {begin + count}))")
        j = i - begin
        if self._torch is not None:
            L = int(self._hist[5][j].item())
            h = self._hist[4][j, :L].cpu().numpy()
        else:
            L = int(self._hist[5][j])
            h = self._hist[4][j, :L]
        out = {}
        for key, (c, w) in HISTORY_CHANNELS.items():
            out[key] = h[:, c:c + w].astype(np.float64) if w else h[:, c].astype(np.float64)
        out["state_history"] = h[:, H_STATE].astype(np.int64)
        return out

    def step(self, actions):
        outputs = (self._actions_in(actions, (self.num_envs, 3)), self._obs, self._rew, self._term, self._trunc, self._fin,
                   self._inner)
        if self._hist is None:
            self._call("salp_robot_vec_step", *outputs, what="step")
        else:
            self._call("salp_robot_vec_step_history", *outputs, *self._hist, what="step")
        term, trunc = self._bool_view(self._term), self._bool_view(self._trunc)
        info = {"inner_steps": self._inner, "final_observation": self._fin, "_final_observation": term | trunc}
        if self._hist is not None:
            info["cycle_history"], info["cycle_history_len"] = self._hist[4], self._hist[5]
            info["cycle_history_envs"] = (self._hist[0], self._hist[1])
        return self._obs, self._rew, term, trunc, info

    # ------------------------------------------------------------------ rollouts: H cycles per robot in one launch
    def _buf(self, name, shape, dtype):
        """The env-owned rollout buffer of that name, made again when its shape changes (H)."""
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape):
            b = self._bufs[name] = self._empty(shape, dtype)
        return b

    def _rollout_outputs(self, H):
        n = self.num_envs
        return (self._buf("obs", (H, n, 6), np.float32), self._buf("reward", (H, n), np.float32),
                self._buf("terminated", (H, n), np.uint8), self._buf("truncated", (H, n), np.uint8),
                self._buf("final_obs", (H, n, 6), np.float32), self._buf("inner_steps", (H, n), np.int32))

    def _rollout_result(self, obs, rew, term, trunc, fin, inner, **extra):
        term, trunc = self._bool_view(term), self._bool_view(trunc)
        return dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_observation=fin,
                    _final_observation=term | trunc, inner_steps=inner, **extra)

    def rollout(self, actions) -> dict:
        """`H` env steps — H breathing cycles of every robot — in ONE kernel launch (salp_robot_vec_rollout): `actions`
        [H, N, 3] in the Box.  Returns a dict of time-major blocks, step t holding what `step(actions[t])` returns:
        `obs` [H, N, 6], `reward` [H, N], `terminated`, `truncated` (bool [H, N]), `final_observation` [H, N, 6] (rows
        where `_final_observation` is set; the others keep what the buffer held), `_final_observation`, `inner_steps`
        int32 [H, N].  The blocks are the env's own buffers, cached per H and overwritten by the next rollout.  In the
        kernel a robot begins its next cycle when its own cycle has ended; results equal the loop of `step` calls up to
        the coupling of a wavefront's lanes (include/salp_robot_rollout.h, < 1e-12 relative per cycle)."""
        H = int(actions.shape[0]) if hasattr(actions, "shape") else len(actions)
        a = self._actions_in(actions, (H, self.num_envs, 3))
        out = self._rollout_outputs(H)
        self._call("salp_robot_vec_rollout", a, H, *out, what="rollout")
        return self._rollout_result(*out)

    def make_policy(self, policy, weights=None) -> "RobotPolicyHandle":
        """An in-kernel policy of this env for `rollout_policy`: a `policy.MLPPolicy` with obs_dim 6 and act_dim 3, one
        policy or a population (P policies share the envs in runs of N / P, whole wavefronts each), or a
        `policy.GaussianPolicy` of those dimensions (salp_robot_policy_create_gaussian: `rollout_policy(..., sample=True)`
        samples from it, `sample=False` runs its mean).
        `MLPPolicy.from_actor(actor)` / `GaussianPolicy.from_actor(actor)` of a `sac.Actor` built with this env's Box
        carries the right scale and shift.
        `handle.update(w)` takes new weights of the same shape in the public layout (`policy.pack()`); with a device
        tensor it is stream-ordered and allocates nothing."""
        gauss = bool(getattr(policy, "gaussian", False))
        self._check_policy(policy)
        p = ctypes.c_void_p()
        w = policy.pack() if weights is None else weights
        _capi.call(self.L, "salp_robot_policy_create_gaussian" if gauss else "salp_robot_policy_create", self._h,
                   ctypes.byref(policy.desc()), w, 0 if weights is None else self._flags, self._stream, ctypes.byref(p),
                   what="make_policy")
        h = RobotPolicyHandle(self, p, policy.n_policies, int(policy.words), gauss)
        self._policies.append(h)
        return h

    def rollout_policy(self, policy, horizon: int, want_actions: bool = True, sample: bool = False) -> dict:
        """`horizon` closed-loop env steps in ONE kernel launch (salp_robot_vec_rollout_policy): every action is `policy`
        applied to the observation row before it — the first one to the env's current observation (`observe()`), the
        action of step t + 1 to `obs[t]`.  `policy`: a handle of `make_policy`, or an `MLPPolicy` (a handle is then made
        and kept for the next call with the same object).  Returns the dict of `rollout` plus `actions` [H, N, 3] (None
        without `want_actions`).
        `sample=True` (salp_robot_vec_rollout_policy_sampled, a `GaussianPolicy` or its handle): every action is the
        tanh-Gaussian sample of include/salp_robot_sampled.h, drawn from the policy's own Philox stream at noise step
        `handle.noise_step` + t; the dict gains `logp` [H, N], and the noise step advances by `horizon` behind the launch.
        `sample=False` on a Gaussian policy runs its mean and leaves the noise step alone.
        Which form is faster (measured on an MI355X, H = 16, DESIGN.md §8f-4 "Rollouts"): at 4096 envs, where every
        wavefront has a SIMD to itself and `step` waits for the slowest env of each launch, the rollout takes 0.53-1.02
        of the time of the loop of actor forward + `step` (the row above 1 lies inside its 7 % spread; open loop
        0.82-0.89); at 262144 envs the loop of `step` calls is the faster form, by 1.5-2.4x: `step` walks the envs
        longest cycle first from 32768 envs on and the rollout does not."""
        handle = self._policy_handle(policy)
        H = int(horizon)
        out = self._rollout_outputs(H)
        aout = self._buf("actions", (H, self.num_envs, 3), np.float32) if want_actions else None
        if sample:
            if not handle.gaussian:
                raise ValueError("sample=True needs a GaussianPolicy (or the handle of one)")
            logp = self._buf("logp", (H, self.num_envs), np.float32)
            self._call("salp_robot_vec_rollout_policy_sampled", handle._p, H, *out, aout, logp, what="rollout_policy (sampled)")
            return self._rollout_result(*out, actions=aout, logp=logp)
        self._call("salp_robot_vec_rollout_policy", handle._p, H, *out, aout, what="rollout_policy")
        return self._rollout_result(*out, actions=aout)

    def evaluate_policy(self, policy, horizon: int, out=None, accumulate: bool = False, sample: bool = False,
                        first_episode: bool = False) -> dict:
        """`horizon` closed-loop env steps of `rollout_policy` in one kernel launch with NO per-step output
        (salp_robot_vec_evaluate_policy, include/salp_robot_evaluate.h): one summary record per robot (48 B) instead of
        seven [H, N] blocks.  Returns typed views of one int32 [N, 12] block (`policy.robot_evaluation_views`): `record`,
        `return_sum` and `first_return` (float64 [N]: the float32 step rewards added in step order in fp64 — over the call,
        and up to the robot's first episode end), `euler_steps` (int64 [N]: Euler steps simulated; seconds = dt x this),
        `first_length`, `first_end` (0 not finished, 1 target reached, 2 truncated), `episodes`, `reached`,
        `first_euler_steps` (int32 [N]).  The record is, bit for bit, `policy.summarize_robot_rollout` of what
        `rollout_policy(policy, horizon)` returns from the same state.
        `out`: a block (or a dict returned earlier) to write into; without it the env uses a block of its own, which the
        next call overwrites.  `accumulate=True` continues the records in the block, so a run cut into several calls (or
        replayed from a captured graph) adds up; an all-zero record is a fresh one, and the env's own block starts zeroed.
        `first_episode=True`: a robot is no longer stepped once its first episode has ended (it sits at the start of its
        next episode), which is how a policy is scored over whole episodes: `evaluate_policy(p, 500, first_episode=True)`.
        With `accumulate`, robots whose record already has `first_end != 0` run nothing.
        `sample=True` (a `GaussianPolicy` or its handle): the run takes the policy's sampled actions, as
        `rollout_policy(..., sample=True)` would; the noise step advances by `horizon` behind the launch."""
        from .policy import REVAL_ACCUMULATE, REVAL_FIRST_EPISODE, REVAL_WORDS, robot_evaluation_views
        handle = self._policy_handle(policy)
        shape = (self.num_envs, REVAL_WORDS)
        if out is None:
            fresh = "record" not in self._bufs
            rec = self._buf("record", shape, np.int32)
            if fresh:
                rec[...] = 0
        else:
            rec = self._out_block(out["record"] if isinstance(out, dict) else out, shape, np.int32)
        views = robot_evaluation_views(rec)       # checks dtype and contiguity
        if sample and not handle.gaussian:
            raise ValueError("sample=True needs a GaussianPolicy (or the handle of one)")
        flags = self._flags | (REVAL_ACCUMULATE if accumulate else 0) | (REVAL_FIRST_EPISODE if first_episode else 0)
        name = "salp_robot_vec_evaluate_policy_sampled" if sample else "salp_robot_vec_evaluate_policy"
        _capi.call(self.L, name, self._h, handle._p, int(horizon), rec, flags, self._stream,
                   what="evaluate_policy (sampled)" if sample else "evaluate_policy")
        return views

    def get_state(self) -> np.ndarray:
        """fp64 [27, N] snapshot, rows R_* (include/salp_robot.h)."""
        s = np.empty((R_COUNT, self.num_envs), np.float64)
        if self._torch is not None:
            self._torch.cuda.current_stream(self.device).synchronize()
        _capi.call(self.L, "salp_robot_vec_get_state", self._h, s, 0, None, what="get_state")
        return s

    def close(self):
        if self._h:
            for p in list(self._policies):     # a policy goes before its handle
                p.close()
            self._policy_cache = {}
            self.L.salp_robot_vec_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
