"""ctypes bindings of the robot evaluation calls' argument checks on the host — TEST INFRASTRUCTURE.

oracle/libsalp_robot_evaluate_host.so is tests/robot_evaluate_host.cpp: csrc/salp_robot_params.h compiled as plain C++ by
the pattern rule of oracle/Makefile.  What salp_robot_vec_evaluate_policy and salp_robot_vec_evaluate_policy_sampled
decide before they touch a GPU is callable here without one: check_evaluate_args() and the constants of
include/salp_robot_evaluate.h.
"""
import ctypes

import native_lib
from native_lib import cint, i32, i64, ptr, text, u32, u64

# every function tests/robot_evaluate_host.cpp exports, in its order
PROTOTYPES = {
    "salp_robot_evaluate_host_check": (cint, [i64, i32, u32, u64, cint, cint, cint, text, cint]),
    "salp_robot_evaluate_host_flags": (None, [ptr(u32)]),
    "salp_robot_evaluate_host_words": (None, [ptr(i32)]),
}
WORD_NAMES = ("RETURN", "FIRST_RETURN", "EULER_STEPS", "FIRST_LENGTH", "FIRST_END", "EPISODES", "REACHED", "FIRST_EULER_STEPS",
              "WORDS")


def lib():
    return native_lib.load("libsalp_robot_evaluate_host.so", PROTOTYPES)


def check_evaluate(max_steps, horizon, flags=0, rec=0x1000, own_policy=True, sampled=False, gaussian=False, msg_size=200):
    """(status, message) of check_evaluate_args(); `rec` is an address (0: NULL)."""
    msg = ctypes.create_string_buffer(msg_size)
    rc = lib().salp_robot_evaluate_host_check(max_steps, horizon, flags, rec, int(own_policy), int(sampled), int(gaussian), msg,
                                              msg_size)
    return rc, msg.value.decode()


def flags() -> dict:
    out = (ctypes.c_uint32 * 3)()
    lib().salp_robot_evaluate_host_flags(out)
    return dict(zip(("DEVICE_PTRS", "ACCUMULATE", "FIRST_EPISODE"), (int(v) for v in out)))


def words() -> dict:
    out = (ctypes.c_int32 * 9)()
    lib().salp_robot_evaluate_host_words(out)
    return dict(zip(WORD_NAMES, (int(v) for v in out)))
