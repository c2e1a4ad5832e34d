"""ctypes bindings of the in-kernel policy's layout functions on the host — TEST INFRASTRUCTURE.

oracle/libsalp_policy_host.so is tests/policy_host.cpp: the host sections of csrc/salp_policy.h and csrc/salp_params.h
compiled as plain C++.  What salp_policy_create and salp_vec_set_state decide before they touch a GPU is callable here
without one: check_policy_desc(), policy_block_map(), policy_header(), policy_bytes() and check_snapshot().
"""
import ctypes

import numpy as np

import native_lib
from native_lib import cint, dbl, i32, i64, ptr, text, u64, vp
from underwater_swimmer_rl_amd.policy import CPolicyDesc


# every function tests/policy_host.cpp exports, in its order
PROTOTYPES = {
    "salp_policy_host_header_words": (cint, []),
    "salp_policy_host_header_slots": (None, [ptr(i32)]),
    "salp_policy_host_check": (cint, [cint, cint, cint, i64, ptr(CPolicyDesc), cint, ptr(cint), ptr(text)]),
    "salp_policy_host_map": (cint, [cint, cint, ptr(CPolicyDesc), cint, ptr(i32), cint]),
    "salp_policy_host_header": (None, [ptr(CPolicyDesc), cint, i64, cint, ptr(i32)]),
    "salp_policy_host_bytes": (None, [ptr(CPolicyDesc), cint, cint, ptr(u64)]),
    "salp_policy_host_check_snapshot": (cint, [i64, vp, vp, text, cint]),
    "salp_policy_host_max_angle": (dbl, []),
}


def lib():
    return native_lib.load("libsalp_policy_host.so", PROTOTYPES)


def desc(n_hidden=0, hidden=(0, 0), out=0, P=1, size=None) -> CPolicyDesc:
    """A salp_policy_desc_t, field by field (size None: the struct's own size)."""
    d = CPolicyDesc()
    d.struct_size = ctypes.sizeof(CPolicyDesc) if size is None else size
    d.n_hidden, d.out_activation, d.n_policies = n_hidden, out, P
    d.hidden[0], d.hidden[1] = hidden
    return d


def desc_of(hidden=(), out=0, P=1) -> CPolicyDesc:
    """The descriptor of a policy with these hidden widths."""
    return desc(len(hidden), tuple(hidden) + (0,) * (2 - len(hidden)), out, P)


def header_slots() -> dict:
    """The header's word indices by name, and WORDS."""
    v = (ctypes.c_int32 * 9)()
    lib().salp_policy_host_header_slots(v)
    names = ("NHIDDEN", "H0", "H1", "OUT", "STRIDE", "GROUP", "COUNT", "GAUSS", "NOISE")
    return dict(zip(names, v), WORDS=lib().salp_policy_host_header_words())


def check(d, obs_dim=24, act_dim=1, kmax=3, n_envs=256, gaussian=False):
    """(status, public words or None, message) of check_policy_desc(); d None is the NULL descriptor."""
    words, why = ctypes.c_int(-1), ctypes.c_char_p()
    rc = lib().salp_policy_host_check(obs_dim, act_dim, kmax, n_envs, None if d is None else ctypes.byref(d), int(gaussian),
                                      ctypes.byref(words), ctypes.byref(why))
    return rc, (words.value if rc == 0 else None), why.value.decode()


def block_map(d, obs_dim=24, act_dim=1, gaussian=False) -> np.ndarray:
    """policy_block_map(): int32 [stride]."""
    stride = lib().salp_policy_host_map(obs_dim, act_dim, ctypes.byref(d), int(gaussian), None, 0)
    m = np.full(stride, -2, np.int32)
    assert lib().salp_policy_host_map(obs_dim, act_dim, ctypes.byref(d), int(gaussian),
                                      m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), stride) == stride
    return m


def header(d, stride, n_envs, gaussian=False) -> np.ndarray:
    """policy_header(): int32 [PH_WORDS]."""
    hd = np.full(lib().salp_policy_host_header_words(), -2, np.int32)
    lib().salp_policy_host_header(ctypes.byref(d), stride, n_envs, int(gaussian), hd.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return hd


def alloc_bytes(d, words, stride) -> tuple:
    """policy_bytes(): the byte counts (block, pub, map) of a policy object's three device allocations."""
    b = (ctypes.c_uint64 * 3)()
    lib().salp_policy_host_bytes(ctypes.byref(d), words, stride, b)
    return tuple(int(v) for v in b)


def check_snapshot(n, f64, i32):
    """(status, message) of check_snapshot() on float64 [rows, n] / int32 [rows, n] (either may be None)."""
    msg = ctypes.create_string_buffer(200)
    for a, t in ((f64, np.float64), (i32, np.int32)):
        assert a is None or (a.dtype == t and a.flags.c_contiguous and a.shape[1] == n)
    rc = lib().salp_policy_host_check_snapshot(n, None if f64 is None else f64.ctypes.data, None if i32 is None else i32.ctypes.data,
                                               msg, len(msg))
    return rc, msg.value.decode()


def max_angle() -> float:
    return lib().salp_policy_host_max_angle()
