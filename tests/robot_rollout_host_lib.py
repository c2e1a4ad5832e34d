"""ctypes bindings of the robot rollout's argument checks on the host — TEST INFRASTRUCTURE.

tests/robot_rollout_host.cpp is csrc/salp_robot_params.h compiled as plain C++ (g++, the flags of oracle/Makefile's host
twins; the library is built next to them, into oracle/).  What salp_robot_vec_rollout and salp_robot_vec_rollout_policy
decide before they touch a GPU is callable here without one: check_rollout_args(), rollout_max_iters() and the constants.
"""
import ctypes
import os
import subprocess

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_ROOT, "tests", "robot_rollout_host.cpp")
_SO = os.path.join(_ROOT, "oracle", "libsalp_robot_rollout_host.so")
CXXFLAGS = ["-O2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(_ROOT, "include", "salp_robot.h"), os.path.join(_ROOT, "include", "salp_robot_rollout.h"),
                os.path.join(_ROOT, "include", "salp_vec.h"),
                os.path.join(_ROOT, "underwater-swimmer_rl_amd", "csrc", "salp_robot_params.h")]
        if not os.path.isfile(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-shared", "-o", _SO, _SRC, "-lm"], check=True)
        L = ctypes.CDLL(_SO)
        i64, i32, u32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
        L.salp_robot_rollout_host_check.argtypes = [i64, i32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.salp_robot_rollout_host_max_iters.argtypes = [i32, i64, ctypes.c_int]
        L.salp_robot_rollout_host_max_iters.restype = i64
        L.salp_robot_rollout_host_max_steps.argtypes = [ctypes.c_double]
        L.salp_robot_rollout_host_max_steps.restype = i64
        L.salp_robot_rollout_host_periods.argtypes = [ctypes.POINTER(i32), ctypes.c_int, ctypes.POINTER(i32)]
        _lib = L
    return _lib


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
