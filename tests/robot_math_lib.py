"""ctypes bindings of the robot kernels' fp64 primitives — TEST INFRASTRUCTURE.

host(function, ...)    oracle/libsalp_robot_math_host.so: tests/robot_math_host.cpp, csrc/salp_fp64_math.h compiled for the host
device(function, ...)  salp_robot_math_probe of libsalp_hip.so: the same header on the GPU, element i on thread i
Both take and return float64 arrays in the layouts listed in csrc/salp_fp64_math.h.
"""
import ctypes

import numpy as np

import native_lib
from native_lib import cint, dbl, i32, i64, vp

SINCOS_SMALL, SINCOS_EULER, ROTATE, CHAIN, RCP_NR, SQRT_NR = range(6)
_ROWS_OUT = {SINCOS_SMALL: 2, SINCOS_EULER: 2, ROTATE: 2, CHAIN: 3, RCP_NR: 1, SQRT_NR: 1}
WAVE = 64

# every function tests/robot_math_host.cpp exports, in its order
PROTOTYPES = {
    "salp_math_host_rotate_max_step": (dbl, []),
    "salp_math_host_euler_fold_above": (dbl, []),
    "salp_math_host": (cint, [cint, vp, vp, i64, i32, vp]),
}


def lib():
    return native_lib.load("libsalp_robot_math_host.so", PROTOTYPES)


def rotate_max_step() -> float:
    """kRotateMaxStep of the header: the largest increment the carried sin / cos take without the exact path."""
    return lib().salp_math_host_rotate_max_step()


def euler_fold_above() -> float:
    return lib().salp_math_host_euler_fold_above()


def _args(function, arrays, steps):
    a = np.ascontiguousarray(np.stack([np.asarray(x, np.float64) for x in arrays]) if isinstance(arrays, (list, tuple))
                             else np.asarray(arrays, np.float64))
    a = a.reshape(-1, a.shape[-1])
    n = a.shape[1]
    want = {SINCOS_SMALL: 1, SINCOS_EULER: 1, ROTATE: 3, CHAIN: 1 + steps, RCP_NR: 1, SQRT_NR: 1}[function]
    assert a.shape[0] == want, (a.shape, want)
    return a, n, np.empty((_ROWS_OUT[function], n), np.float64)


def host(function, arrays, steps=0, want_exact_steps=False):
    """Rows of the result ([2][n], [3][n] for CHAIN).  CHAIN: `arrays` is [1 + steps][n] (start angles, then increments);
    with want_exact_steps also the [steps][groups of 64] map of the steps on which a group took the exact path."""
    a, n, out = _args(function, arrays, steps)
    ex = np.zeros((steps, (n + WAVE - 1) // WAVE), np.uint8) if want_exact_steps else None
    rc = lib().salp_math_host(function, a.ctypes.data, out.ctypes.data, n, steps, None if ex is None else ex.ctypes.data)
    assert rc == 0, rc
    return (out, ex) if want_exact_steps else out


def device(function, arrays, steps=0, device_id=0):
    from underwater_swimmer_rl_amd import _capi
    L = _capi.load_library()
    L.salp_robot_math_probe.argtypes = [cint, cint, vp, vp, i64, i32]
    L.salp_robot_last_error.restype = ctypes.c_char_p
    a, n, out = _args(function, arrays, steps)
    rc = L.salp_robot_math_probe(device_id, function, a.ctypes.data, out.ctypes.data, n, steps)
    assert rc == 0, L.salp_robot_last_error()
    return out
