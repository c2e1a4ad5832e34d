"""ctypes bindings of the robot rollout's argument checks on the host — TEST INFRASTRUCTURE.

oracle/libsalp_robot_rollout_host.so is tests/robot_rollout_host.cpp: csrc/salp_robot_params.h compiled as plain C++.  What
salp_robot_vec_rollout and salp_robot_vec_rollout_policy decide before they touch a GPU is callable here without one:
check_rollout_args(), rollout_max_iters() and the constants.
"""
import ctypes

import native_lib
from native_lib import cint, dbl, i32, i64, ptr, text, u32

# every function tests/robot_rollout_host.cpp exports, in its order
PROTOTYPES = {
    "salp_robot_rollout_host_check": (cint, [i64, i32, u32, cint, cint, text, cint]),
    "salp_robot_rollout_host_max_cycles": (cint, []),
    "salp_robot_rollout_host_max_iters": (i64, [i32, i64, cint]),
    "salp_robot_rollout_host_max_steps": (i64, [dbl]),
    "salp_robot_rollout_host_periods": (cint, [ptr(i32), cint, ptr(i32)]),
}


def lib():
    return native_lib.load("libsalp_robot_rollout_host.so", PROTOTYPES)


def check_rollout(max_steps, horizon, flags=0, source=True, main_output=True, msg_size=200):
    """(status, message) of check_rollout_args()."""
    msg = ctypes.create_string_buffer(msg_size)
    rc = lib().salp_robot_rollout_host_check(max_steps, horizon, flags, int(source), int(main_output), msg, msg_size)
    return rc, msg.value.decode()


def max_cycles() -> int:
    return lib().salp_robot_rollout_host_max_cycles()


def max_iters(horizon, max_steps, period) -> int:
    return lib().salp_robot_rollout_host_max_iters(horizon, max_steps, period)


def max_steps(dt: float) -> int:
    return lib().salp_robot_rollout_host_max_steps(dt)


def periods():
    """(kRolloutPeriods as a tuple, kRolloutPeriod)."""
    out, shipped = (ctypes.c_int32 * 16)(), ctypes.c_int32(-1)
    count = lib().salp_robot_rollout_host_periods(out, 16, ctypes.byref(shipped))
    return tuple(out[:count]), shipped.value
