"""ctypes bindings of the robot kernels' fp64 primitives — TEST INFRASTRUCTURE.

host(function, ...)    oracle/libsalp_math_host.so: tests/robot_math_host.cpp, csrc/salp_fp64_math.h compiled for the host
device(function, ...)  salp_robot_math_probe of libsalp_hip.so: the same header on the GPU, element i on thread i
Both take and return float64 arrays in the layouts listed in csrc/salp_fp64_math.h.
"""
import ctypes
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "oracle", "libsalp_math_host.so")

SINCOS_SMALL, SINCOS_EULER, ROTATE, CHAIN, RCP_NR, SQRT_NR = range(6)
_ROWS_OUT = {SINCOS_SMALL: 2, SINCOS_EULER: 2, ROTATE: 2, CHAIN: 3, RCP_NR: 1, SQRT_NR: 1}
WAVE = 64

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(_ROOT, "tests", "robot_math_host.cpp"),
                os.path.join(_ROOT, "underwater-swimmer_rl_amd", "csrc", "salp_fp64_math.h")]
        if not os.path.isfile(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["make", "-C", os.path.join(_ROOT, "oracle"), "-s", "libsalp_math_host.so"], check=True)
        L = ctypes.CDLL(_SO)
        vp = ctypes.c_void_p
        L.salp_math_host.argtypes = [ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int32, vp]
        L.salp_math_host_rotate_max_step.restype = ctypes.c_double
        L.salp_math_host_euler_fold_above.restype = ctypes.c_double
        _lib = L
    return _lib


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
    vp = ctypes.c_void_p
    L.salp_robot_math_probe.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int32]
    L.salp_robot_last_error.restype = ctypes.c_char_p
    a, n, out = _args(function, arrays, steps)
    rc = L.salp_robot_math_probe(device_id, function, a.ctypes.data, out.ctypes.data, n, steps)
    assert rc == 0, L.salp_robot_last_error()
    return out
