"""Batched trajectory comparison for the HEAD simulator: the reference's
`compare_actions_with_states(actions, expected_states, robot)` (src/salp/environments/compare_trajectories.py:19-117)
for N candidate robots at once, each with its own physical parameters (salp_robot_vec_trajectory,
include/salp_robot.h).  Fitting the model to a measured run is then one call per batch of candidates:

    P = robot_params(65536, "cuda:0", drag_coefficient_max=torch.rand(65536, device="cuda:0") + 0.5)
    out = compare_actions_with_states(actions, measured, P, metrics_only=True)      # actions [T, 3] in m, s, rad
    best = out["position_error"].argmin()

Actions are fp64 in the reference's physical units (contraction m, coast time s, nozzle yaw rad), not the env's Box.
Results are float64 tensors on the device, batched along a new leading robot axis."""
from __future__ import annotations

import ctypes
import threading

from . import _capi
from .robot_env import CRobotConfig, SalpRobotVectorEnv

# rows of the parameter table, SALP_RP_* of include/salp_robot.h (names = salp_robot_config_t fields)
ROBOT_PARAM_NAMES = ("dry_mass", "init_length", "init_width", "max_contraction", "density", "drag_coefficient_min",
                     "drag_coefficient_max", "nozzle_length1", "nozzle_length2", "nozzle_area", "nozzle_mass",
                     "nozzle_gamma")
# columns of the kernel's metrics, SALP_RM_* (the reference's return keys, plus the mean |d yaw rate|)
METRIC_NAMES = ("position_error", "velocity_error", "angle_error", "max_position_error", "angular_velocity_error")
PER_ROBOT_ACTIONS = 2          # SALP_ROBOT_PER_ROBOT_ACTIONS
MAX_TRAJECTORY_CYCLES = 1024   # SALP_ROBOT_MAX_TRAJECTORY_CYCLES


def _default_config() -> CRobotConfig:
    cfg = CRobotConfig()
    _capi.call(_capi.load_library(), "salp_robot_config_default", ctypes.byref(cfg))
    return cfg


def robot_params(n: int, device="cuda:0", **overrides):
    """float64 [len(ROBOT_PARAM_NAMES), n] table: salp_robot_config_default's values, with each override (a scalar or
    a length-n vector) in its row."""
    import torch
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    cfg = _default_config()
    table = torch.empty((len(ROBOT_PARAM_NAMES), n), dtype=torch.float64, device=device)
    for j, name in enumerate(ROBOT_PARAM_NAMES):
        table[j] = getattr(cfg, name)
    for name, v in overrides.items():
        if name not in ROBOT_PARAM_NAMES:
            raise TypeError(f"unknown robot parameter {name!r} (one of {', '.join(ROBOT_PARAM_NAMES)})")
        v = torch.as_tensor(v, dtype=torch.float64).to(device)
        if v.dim() > 1 or (v.dim() == 1 and v.shape[0] != n):
            raise ValueError(f"{name}: expected a scalar or a vector of length {n}, got shape {tuple(v.shape)}")
        table[ROBOT_PARAM_NAMES.index(name)] = v
    return table


def params_from_robot(robot) -> dict:
    """The parameters of a reference `Robot` (robot.py), read by duck typing, as keyword overrides for robot_params:
    Robot(dry_mass, init_length, init_width, max_contraction, nozzle), set_environment(density), _drag_coefficents
    and Nozzle(length1, length2, area, mass) / nozzle.gamma."""
    nz = robot.nozzle
    cd_min, cd_max = robot._drag_coefficents
    vals = dict(dry_mass=robot.dry_mass, init_length=robot.init_length, init_width=robot.init_width,
                max_contraction=robot.max_contraction, density=robot.density, drag_coefficient_min=cd_min,
                drag_coefficient_max=cd_max, nozzle_length1=nz.length1, nozzle_length2=nz.length2, nozzle_area=nz.area,
                nozzle_mass=nz.mass, nozzle_gamma=nz.gamma)
    return {k: float(vals[k]) for k in ROBOT_PARAM_NAMES}


_handles = threading.local()


def _handle(n: int, device):
    """One robot-env handle per (n, device) and thread, reused across calls: the trajectory call does not touch its
    env state, only its config (dt) and its staging buffer."""
    cache = getattr(_handles, "cache", None)
    if cache is None:
        cache = _handles.cache = {}
    key = (n, str(device))
    if key not in cache:
        if len(cache) >= 4:
            for k in list(cache):
                cache.pop(k).close()
        cache[key] = SalpRobotVectorEnv(n, device=str(device), seed=0, output="torch")
    return cache[key]


def compare_actions_with_states(actions, expected_states=None, params=None, *, num_robots=None, device="cuda:0",
                                metrics_only=False) -> dict:
    """compare_actions_with_states of compare_trajectories.py for N robots.

    actions          [T, 3] shared by every robot, or [N, T, 3] per robot (contraction m, coast time s, yaw rad)
    expected_states  [T, 6] (x, y, body vx, vy, yaw, yaw rate) or None
    params           None (every robot is the default robot), a [12, N] table (robot_params), a dict of overrides,
                     or a reference `Robot` (params_from_robot)
    num_robots       N when neither params nor actions give it (default 1)
    metrics_only     only the kernel's per-robot metrics: no per-cycle data is written

    Returns the reference's keys with a leading robot axis: actual_states [N, T, 6], expected_states [T, 6], errors
    [N, T, 6], position_errors / velocity_errors / angle_errors [N, T] (computed here from the states), position_error,
    velocity_error, angle_error, max_position_error [N] (computed by the kernel), plus angular_velocity_error [N]
    (mean |d yaw rate|) and inner_steps [N, T] (Euler steps per cycle).  Without expected_states only actual_states
    and inner_steps."""
    import torch
    dev = torch.device(device)
    a = torch.as_tensor(actions, dtype=torch.float64).to(dev)
    if a.dim() == 2 and a.shape[1] == 3:
        per_robot, T = False, a.shape[0]
    elif a.dim() == 3 and a.shape[2] == 3:
        per_robot, T = True, a.shape[1]
    else:
        raise ValueError(f"actions must be [T, 3] or [N, T, 3], got shape {tuple(a.shape)}")
    if params is not None and not isinstance(params, dict) and hasattr(params, "nozzle"):
        params = params_from_robot(params)
    sizes = set()
    if per_robot:
        sizes.add(a.shape[0])
    if params is not None and not isinstance(params, dict):
        params = torch.as_tensor(params, dtype=torch.float64).to(dev)
        if params.dim() != 2 or params.shape[0] != len(ROBOT_PARAM_NAMES):
            raise ValueError(f"params must be [{len(ROBOT_PARAM_NAMES)}, N], got shape {tuple(params.shape)}")
        sizes.add(params.shape[1])
    if num_robots is not None:
        sizes.add(int(num_robots))
    if len(sizes) > 1:
        raise ValueError(f"inconsistent robot counts {sorted(sizes)} (actions, params, num_robots)")
    n = sizes.pop() if sizes else 1
    if isinstance(params, dict):
        params = robot_params(n, dev, **params)
    if expected_states is None and metrics_only:
        raise ValueError("metrics_only needs expected_states")
    x = None
    if expected_states is not None:
        x = torch.as_tensor(expected_states, dtype=torch.float64).to(dev)
        if tuple(x.shape) != (T, 6):
            raise ValueError(f"expected_states must be [{T}, 6], got shape {tuple(x.shape)}")
        x = x.contiguous()
    if per_robot:
        a = a.transpose(0, 1)          # [T, N, 3], the kernel's layout
    a = a.contiguous()
    if params is not None:
        params = params.contiguous()

    env = _handle(n, dev)
    states = None if metrics_only else torch.empty((T, n, 6), dtype=torch.float64, device=dev)
    inner = None if metrics_only else torch.empty((T, n), dtype=torch.int32, device=dev)
    metrics = None if x is None else torch.empty((n, len(METRIC_NAMES)), dtype=torch.float64, device=dev)
    flags = 1 | (PER_ROBOT_ACTIONS if per_robot else 0)
    _capi.call(env.L, "salp_robot_vec_trajectory", env._h, params, a, int(T), x, states, metrics, inner, flags, env._stream)
    out = {}
    if states is not None:
        out["actual_states"] = states.transpose(0, 1)
        out["inner_steps"] = inner.transpose(0, 1)
    if x is not None:
        out["expected_states"] = x
        if states is not None:
            err = out["actual_states"] - x
            out["errors"] = err
            out["position_errors"] = torch.linalg.vector_norm(err[..., 0:2], dim=-1)
            out["velocity_errors"] = torch.linalg.vector_norm(err[..., 2:4], dim=-1)
            out["angle_errors"] = err[..., 4].abs()
        for j, name in enumerate(METRIC_NAMES):
            out[name] = metrics[:, j]
    return out


__all__ = ["ROBOT_PARAM_NAMES", "METRIC_NAMES", "robot_params", "params_from_robot", "compare_actions_with_states"]
