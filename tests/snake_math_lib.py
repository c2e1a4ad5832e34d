"""ctypes binding of the snake step's math probe — TEST INFRASTRUCTURE.

device(function, rows, cfg=None, seed=0)  salp_snake_math_probe of libsalp_hip.so (csrc/salp_snake_math_probe.h): one of the
primitives of csrc/salp_snake_math.h, csrc/salp_philox.h or jet_thrust_terms (csrc/salp_step.h) on the GPU, element i on
thread i.  Rows in and out are float64 [rows][n]; fp32 and uint32 values travel exactly inside doubles.  The probe is not
part of the public ABI, so the prototype is set here and not in _capi.PROTOTYPES.
"""
import ctypes

import numpy as np

(SINCOS_T, SIN_NOZZLE_T, ATAN2, ATAN2_PRECISE, COS_WRAPPED, REL_HEADING, REL_HEADING_PRECISE, PHILOX, U53, THRUST_STD,
 THRUST_RT) = range(11)
ROWS_IN = {SINCOS_T: 1, SIN_NOZZLE_T: 1, ATAN2: 2, ATAN2_PRECISE: 2, COS_WRAPPED: 1, REL_HEADING: 3, REL_HEADING_PRECISE: 3,
           PHILOX: 6, U53: 2, THRUST_STD: 7, THRUST_RT: 7}
ROWS_OUT = {SINCOS_T: 2, SIN_NOZZLE_T: 1, ATAN2: 1, ATAN2_PRECISE: 1, COS_WRAPPED: 1, REL_HEADING: 1, REL_HEADING_PRECISE: 1,
            PHILOX: 4, U53: 1, THRUST_STD: 7, THRUST_RT: 7}


def library():
    """libsalp_hip.so with the probe's prototype declared."""
    from underwater_swimmer_rl_amd import _capi
    from underwater_swimmer_rl_amd.config import CConfig
    L = _capi.load_library()
    vp = ctypes.c_void_p
    L.salp_snake_math_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(CConfig), ctypes.c_uint64, vp, vp, ctypes.c_int64]
    L.salp_snake_math_probe.restype = ctypes.c_int
    L.salp_last_error.restype = ctypes.c_char_p
    return L


def device(function, rows, cfg=None, seed=0, device_id=0):
    """`rows`: one array or a list of ROWS_IN[function] arrays of n values.  `cfg`: a SalpSnakeConfig (None = the defaults, a
    NULL config).  Returns float64 [ROWS_OUT[function]][n]."""
    L = library()
    a = np.ascontiguousarray(np.stack([np.asarray(x, np.float64) for x in rows]) if isinstance(rows, (list, tuple))
                             else np.asarray(rows, np.float64))
    a = a.reshape(-1, a.shape[-1])
    assert a.shape[0] == ROWS_IN[function], (a.shape, ROWS_IN[function])
    n = a.shape[1]
    out = np.empty((ROWS_OUT[function], n), np.float64)
    c = None if cfg is None else ctypes.byref(cfg.to_c())
    rc = L.salp_snake_math_probe(device_id, function, c, seed, a.ctypes.data, out.ctypes.data, n)
    assert rc == 0, (rc, L.salp_last_error())
    return out
