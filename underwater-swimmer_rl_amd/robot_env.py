"""Batched HEAD simulator: the reference's `SalpRobotEnv(robot=Robot(...))`
(src/salp/environments/salp_robot_env.py over robot.py) for N robots on one MI355X.

    env = SalpRobotVectorEnv(num_envs=65536, device="cuda:0", seed=0)
    obs, _ = env.reset()
    obs, reward, terminated, truncated, info = env.step(actions)      # actions [N, 3] in [0,1]x[0,1]x[-1,1]

One `step` is one whole breathing cycle of every robot (Robot.set_control + step_through_cycle,
robot.py:335-358, 422-445): `info["inner_steps"]` is the number of Euler steps each robot took.
`env.record_history(slice(a, b), stride)` adds the per-Euler-step history of those robots to `info`
(`cycle_history`, `cycle_history_len`, `cycle_history_envs`; `env.history_of(i)` in the reference's shape).
Same conventions as SalpVectorEnv: device tensors, same-step autoreset with `final_observation`,
no CPU fallback."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _capi
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

ROBOT_EXPORTS = ("salp_robot_last_error", "salp_robot_config_default", "salp_robot_vec_create", "salp_robot_vec_destroy",
                 "salp_robot_vec_num_envs", "salp_robot_vec_reset", "salp_robot_vec_step", "salp_robot_vec_get_state",
                 "salp_robot_vec_history_capacity", "salp_robot_vec_step_history", "salp_robot_vec_trajectory")


class CRobotConfig(ctypes.Structure):
    """salp_robot_config_t (include/salp_robot.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("tank_margin", ctypes.c_double), ("dry_mass", ctypes.c_double), ("init_length", ctypes.c_double),
                ("init_width", ctypes.c_double), ("max_contraction", ctypes.c_double), ("density", ctypes.c_double),
                ("dt", ctypes.c_double), ("drag_coefficient_min", ctypes.c_double), ("drag_coefficient_max", ctypes.c_double),
                ("nozzle_length1", ctypes.c_double), ("nozzle_length2", ctypes.c_double), ("nozzle_length3", ctypes.c_double),
                ("nozzle_area", ctypes.c_double), ("nozzle_mass", ctypes.c_double), ("nozzle_gamma", ctypes.c_double),
                ("max_cycles", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


def _lib():
    L = _capi.load_library()
    if not getattr(L, "_salp_robot_ready", False):
        vp, i64, u64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32
        L.salp_robot_last_error.restype = ctypes.c_char_p
        L.salp_robot_config_default.argtypes = [ctypes.POINTER(CRobotConfig)]
        L.salp_robot_vec_create.argtypes = [ctypes.POINTER(CRobotConfig), i64, ctypes.c_int, u64, i64, ctypes.POINTER(vp)]
        L.salp_robot_vec_destroy.argtypes = [vp]
        L.salp_robot_vec_destroy.restype = None
        L.salp_robot_vec_num_envs.argtypes = [vp]
        L.salp_robot_vec_num_envs.restype = i64
        L.salp_robot_vec_reset.argtypes = [vp, vp, vp, u32, vp]
        L.salp_robot_vec_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
        L.salp_robot_vec_get_state.argtypes = [vp, vp, u32, vp]
        L.salp_robot_vec_history_capacity.argtypes = [vp, ctypes.c_int32]
        L.salp_robot_vec_history_capacity.restype = ctypes.c_int32
        L.salp_robot_vec_step_history.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_int32, ctypes.c_int32,
                                                  vp, vp, u32, vp]
        L.salp_robot_vec_trajectory.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp, u32, vp]
        L._salp_robot_ready = True
    return L


def _check(L, rc, what):
    if rc != 0:
        raise _capi.SalpError(f"{what} failed ({rc}): {L.salp_robot_last_error().decode()}")


class SalpRobotVectorEnv:
    def __init__(self, num_envs: int = 4096, device="cuda:0", seed: int = 0, env_index_base: int = 0,
                 output: str = "torch", **robot_params):
        self.L = _lib()
        self.num_envs = int(num_envs)
        cfg = CRobotConfig()
        _check(self.L, self.L.salp_robot_config_default(ctypes.byref(cfg)), "salp_robot_config_default")
        for k, v in robot_params.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown robot parameter {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self._dev_index = int(str(device).split(":")[1]) if isinstance(device, str) and ":" in device else int(device) if not isinstance(device, str) else 0
        self._h = ctypes.c_void_p()
        _check(self.L, self.L.salp_robot_vec_create(ctypes.byref(cfg), self.num_envs, self._dev_index, int(seed),
                                                    int(env_index_base), ctypes.byref(self._h)), "salp_robot_vec_create")
        self.obs_dim, self.act_dim = 6, 3
        # salp_robot_env.py:48-69
        self.single_action_space = Box(low=np.array([0.0, 0.0, -1.0]), high=np.array([1.0, 1.0, 1.0]), dtype=np.float32)
        self.single_observation_space = Box(low=np.full(6, -np.inf), high=np.full(6, np.inf), dtype=np.float32)
        self.action_space = batch_space(self.single_action_space, self.num_envs)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        self._torch = None
        if output == "torch":
            import torch
            if not torch.cuda.is_available():
                raise _capi.SalpError("output='torch' needs a ROCm GPU visible to PyTorch")
            self._torch, self.device = torch, torch.device("cuda", self._dev_index)
        n = self.num_envs
        self._obs, self._fin = self._new((n, 6), np.float32), self._new((n, 6), np.float32)
        self._rew, self._term, self._trunc = self._new((n,), np.float32), self._new((n,), np.uint8), self._new((n,), np.uint8)
        self._inner = self._new((n,), np.int32)
        self._hist = None      # (begin, count, stride, capacity, history, history_len) while record_history is on

    def _new(self, shape, dtype):
        if self._torch is not None:
            td = {np.float32: self._torch.float32, np.uint8: self._torch.uint8, np.int32: self._torch.int32}[dtype]
            return self._torch.empty(shape, dtype=td, device=self.device)
        return np.empty(shape, dtype)

    _p = staticmethod(_capi.SalpLib._ptr)

    @property
    def _flags(self):
        return 1 if self._torch is not None else 0

    @property
    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream) if self._torch is not None else None

    def reset(self, *, seed: Optional[int] = None, options=None, mask=None):
        m = None
        if mask is not None:
            m = (self._torch.as_tensor(mask).to(self.device, self._torch.uint8).contiguous() if self._torch is not None
                 else np.ascontiguousarray(mask, np.uint8))
        _check(self.L, self.L.salp_robot_vec_reset(self._h, self._p(m), self._p(self._obs), self._flags, self._stream), "reset")
        return self._obs, {}

    def observe(self):
        zero = (self._torch.zeros(self.num_envs, dtype=self._torch.uint8, device=self.device) if self._torch is not None
                else np.zeros(self.num_envs, np.uint8))
        _check(self.L, self.L.salp_robot_vec_reset(self._h, self._p(zero), self._p(self._obs), self._flags, self._stream), "observe")
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
        self._hist = (begin, count, int(stride), cap, self._new((count, cap, H_COUNT), np.float32), self._new((count,), np.int32))

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
        if self._torch is not None:
            t = self._torch
            a = actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions, np.float32))
            a = a.to(self.device, t.float32).reshape(self.num_envs, 3).contiguous()
        else:
            a = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(self.num_envs, 3))
        if self._hist is None:
            _check(self.L, self.L.salp_robot_vec_step(self._h, self._p(a), self._p(self._obs), self._p(self._rew), self._p(self._term),
                                                       self._p(self._trunc), self._p(self._fin), self._p(self._inner), self._flags,
                                                       self._stream), "step")
        else:
            begin, count, stride, cap, hist, hlen = self._hist
            _check(self.L, self.L.salp_robot_vec_step_history(
                self._h, self._p(a), self._p(self._obs), self._p(self._rew), self._p(self._term), self._p(self._trunc),
                self._p(self._fin), self._p(self._inner), begin, count, stride, cap, self._p(hist), self._p(hlen), self._flags,
                self._stream), "step")
        if self._torch is not None:
            term, trunc = self._term.view(self._torch.bool), self._trunc.view(self._torch.bool)
        else:
            term, trunc = self._term.view(np.bool_), self._trunc.view(np.bool_)
        info = {"inner_steps": self._inner, "final_observation": self._fin, "_final_observation": term | trunc}
        if self._hist is not None:
            info["cycle_history"], info["cycle_history_len"] = self._hist[4], self._hist[5]
            info["cycle_history_envs"] = (self._hist[0], self._hist[1])
        return self._obs, self._rew, term, trunc, info

    def get_state(self) -> np.ndarray:
        """fp64 [27, N] snapshot, rows R_* (include/salp_robot.h)."""
        s = np.empty((R_COUNT, self.num_envs), np.float64)
        if self._torch is not None:
            self._torch.cuda.current_stream(self.device).synchronize()
        _check(self.L, self.L.salp_robot_vec_get_state(self._h, s.ctypes.data_as(ctypes.c_void_p), 0, None), "get_state")
        return s

    def close(self):
        if self._h:
            self.L.salp_robot_vec_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
