"""ctypes bindings of the wide in-kernel policy's host twin — TEST INFRASTRUCTURE.

oracle/libsalp_wide_policy_host.so is tests/wide_policy_host.cpp: the host section of csrc/salp_policy_wide.h compiled as
plain C++ (ranges, block map, header, the largest index read, the shared constexpr maps), an fmaf restatement of the
promised arithmetic for widths up to 256 written from the public layout alone (`policy_forward`, `policy_forward_gaussian`:
the call shapes of `oracle_lib`'s), and a replay of the kernel's data flow on 64 host lanes (`emulate`).
"""
import ctypes

import numpy as np

import native_lib
from native_lib import cint, i32, i64, ptr, text, vp
from underwater_swimmer_rl_amd.policy import CPolicyDesc

# every function tests/wide_policy_host.cpp exports, in its order
PROTOTYPES = {
    "salp_wide_policy_host_check": (cint, [cint, cint, cint, cint, i64, ptr(CPolicyDesc), cint, ptr(cint), ptr(text)]),
    "salp_wide_policy_host_map": (cint, [cint, ptr(CPolicyDesc), cint, ptr(i32), cint]),
    "salp_wide_policy_host_header": (None, [ptr(CPolicyDesc), cint, i64, cint, ptr(i32)]),
    "salp_wide_policy_host_read_end": (cint, [ptr(CPolicyDesc)]),
    "salp_wide_policy_host_index": (cint, [cint, cint, cint]),
    "salp_wide_policy_forward": (cint, [ptr(CPolicyDesc), i32, vp, vp, i64, vp, vp]),
    "salp_wide_policy_forward_gaussian": (cint, [ptr(CPolicyDesc), i32, vp, vp, i64, vp, vp]),
    "salp_wide_policy_emulate": (cint, [ptr(CPolicyDesc), vp, cint, vp, vp]),
}
CD_ROW, A_WORD, LAST_WORD, BIAS_WORD, TILE_WORDS, REORDER_KSTEP, PH_WIDE, AB_INDEX, AB_K = range(9)
TILE, ROWS, TAIL_WORDS, TAIL_SCALE, TAIL_SHIFT, OBS = 32, 4, 16, 4, 6, 24


def lib():
    return native_lib.load("libsalp_wide_policy_host.so", PROTOTYPES)


def index(code, a=0, b=0) -> int:
    return lib().salp_wide_policy_host_index(code, a, b)


def check(d, obs_dim=24, act_dim=1, kmax=3, food_slots=1, n_envs=256, gaussian=False):
    """(status, public words or None, message) of check_policy_desc_wide(); d None is the NULL descriptor."""
    words, why = ctypes.c_int(-1), ctypes.c_char_p()
    rc = lib().salp_wide_policy_host_check(obs_dim, act_dim, kmax, food_slots, n_envs, None if d is None else ctypes.byref(d),
                                           int(gaussian), ctypes.byref(words), ctypes.byref(why))
    return rc, (words.value if rc == 0 else None), why.value.decode()


def block_map(d, act_dim=1, gaussian=False) -> np.ndarray:
    """policy_block_map_wide(): int32 [stride]."""
    stride = lib().salp_wide_policy_host_map(act_dim, ctypes.byref(d), int(gaussian), None, 0)
    m = np.full(stride, -2, np.int32)
    assert lib().salp_wide_policy_host_map(act_dim, ctypes.byref(d), int(gaussian), m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), stride) == stride
    return m


def header(d, stride, n_envs, gaussian=False) -> np.ndarray:
    hd = np.full(16, -2, np.int32)
    lib().salp_wide_policy_host_header(ctypes.byref(d), stride, n_envs, int(gaussian), hd.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return hd


def read_end(d) -> int:
    return lib().salp_wide_policy_host_read_end(ctypes.byref(d))


def _p(a):
    return a.ctypes.data


def _forward(name, policy, obs, weights):
    x = np.ascontiguousarray(obs, dtype=np.float32)
    P, OD, AD = policy.n_policies, policy.obs_dim, policy.act_dim
    assert OD == OBS and x.shape[-1] == OD
    w = np.ascontiguousarray(policy.pack() if weights is None else weights, dtype=np.float32).reshape(P, policy.words)
    policy.check_envs(x.shape[-2])
    lead, N = x.shape[:-2], x.shape[-2]
    g = np.ascontiguousarray(np.moveaxis(x.reshape(-1, P, N // P, OD), 1, 0))           # [P, L, G, OD]
    u = np.empty(g.shape[:-1] + (AD,), np.float32)
    a = np.empty_like(u)
    d = policy.desc()
    for k in range(P):
        rc = getattr(lib(), name)(ctypes.byref(d), AD, _p(w[k]), _p(g[k]), g[k].size // OD, _p(u[k]), _p(a[k]))
        if rc != 0:
            raise RuntimeError(f"{name} failed: {rc}")
    back = lambda v: np.ascontiguousarray(np.moveaxis(v, 0, 1)).reshape(lead + (N, AD))
    return back(u), back(a)


def policy_forward(policy, obs, weights=None):
    """u (before the output activation) and a, float32 [..., N, act_dim]: `oracle_lib.policy_forward` for widths up to 256."""
    return _forward("salp_wide_policy_forward", policy, obs, weights)


def policy_forward_gaussian(policy, obs, weights=None):
    """m (the mean head) and r (the log-std head's raw sum), float32 [..., N, act_dim]."""
    return _forward("salp_wide_policy_forward_gaussian", policy, obs, weights)


def device_block(policy, k=0) -> np.ndarray:
    """Policy k's words of the device block, float32 [stride]: the public words through the map, zeros elsewhere."""
    m = block_map(policy.desc(), policy.act_dim, bool(getattr(policy, "gaussian", False)))
    w = policy.pack()[k]
    return np.where(m >= 0, w[np.maximum(m, 0)], np.float32(0)).astype(np.float32)


def emulate(policy, obs64, k=0):
    """The kernel's data flow replayed on 64 host lanes: the last layer's four row sums float32 [64, 4] of 64 observation
    rows, and how many words beyond the stride the replay would have read."""
    blk = device_block(policy, k)
    x = np.ascontiguousarray(obs64, np.float32)
    assert x.shape == (64, OBS)
    rows = np.empty((64, ROWS), np.float32)
    d = policy.desc()
    beyond = lib().salp_wide_policy_emulate(ctypes.byref(d), _p(blk), blk.size, _p(x), _p(rows))
    return rows, beyond
