"""ctypes binding of the C ABI in include/salp_vec.h (libsalp_hip.so, built in-tree by
`__graft_entry__.build()` / `csrc/build.py`).

There is no CPU fallback: if the shared library is missing or no HIP device is usable the
constructors raise (`SalpError`), they never route to another implementation.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

from .config import CConfig, SalpSnakeConfig
from .policy import CPolicyDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsalp_hip.so")

SALP_DEVICE_PTRS = 1
INFO_COLS = 3
# packed transition record (include/salp_vec.h "Packed transition record"; layout helpers: records.py)
REC_FINAL_OBS = 2           # call flag next to SALP_DEVICE_PTRS
REC_REWARD, REC_FLAGS, REC_FOOD_COLLECTED, REC_STEPS_SINCE_FOOD, REC_EXTRA_COLS = range(5)
# per-env summary record of salp_vec_evaluate_policy (include/salp_vec.h "Policy evaluation"; views: policy.evaluation_views)
EVAL_ACCUMULATE = 4         # call flag next to SALP_DEVICE_PTRS
EVAL_RETURN, EVAL_FIRST_RETURN, EVAL_FIRST_LENGTH, EVAL_FIRST_END, EVAL_EPISODES, EVAL_FOOD, EVAL_WORDS = 0, 2, 4, 5, 6, 7, 8
# per-env navigation record of salp_vec_evaluate_navigation (include/salp_vec.h "Navigation evaluation"; views: policy.navigation_views)
(NAV_STEPS, NAV_STATUS, NAV_PATH, NAV_LATERAL, NAV_XMIN, NAV_XMAX, NAV_YMIN, NAV_YMAX, NAV_X, NAV_Y,
 NAV_WORDS) = 0, 1, 2, 4, 6, 8, 10, 12, 14, 16, 20
NAV_REACHED, NAV_COLLIDED, NAV_CAPTURED = 1, 2, 4     # bits of NAV_STATUS
# snapshot rows (include/salp_vec.h)
F_X, F_Y, F_VX, F_VY, F_THETA, F_OMEGA, F_NOZZLE, F_WATER, F_ELLIPSE_A, F_ELLIPSE_B, F_FOOD0 = range(11)
(I_PHASE, I_TIMER, I_EXHALE_DUR, I_SHAPE_HOLD, I_STEPS_SINCE_FOOD, I_FOOD_COLLECTED, I_RNG_COUNTER,
 I_EPISODE_LENGTH, I_COUNT) = range(9)

class SalpError(RuntimeError):
    pass


class CStats(ctypes.Structure):
    _fields_ = [
        ("env_steps", ctypes.c_int64), ("episodes", ctypes.c_int64), ("terminated", ctypes.c_int64),
        ("truncated", ctypes.c_int64), ("collisions", ctypes.c_int64), ("food_collected", ctypes.c_int64),
        ("episode_length_sum", ctypes.c_int64), ("reward_sum", ctypes.c_double),
        ("episode_return_sum", ctypes.c_double),
    ]


class CRobotConfig(ctypes.Structure):
    """salp_robot_config_t (include/salp_robot.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("tank_margin", ctypes.c_double), ("dry_mass", ctypes.c_double), ("init_length", ctypes.c_double),
                ("init_width", ctypes.c_double), ("max_contraction", ctypes.c_double), ("density", ctypes.c_double),
                ("dt", ctypes.c_double), ("drag_coefficient_min", ctypes.c_double), ("drag_coefficient_max", ctypes.c_double),
                ("nozzle_length1", ctypes.c_double), ("nozzle_length2", ctypes.c_double), ("nozzle_length3", ctypes.c_double),
                ("nozzle_area", ctypes.c_double), ("nozzle_mass", ctypes.c_double), ("nozzle_gamma", ctypes.c_double),
                ("max_cycles", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


def _prototypes():
    """name -> (restype, argtypes) of every function of include/salp_vec_policy_packed.h, of include/salp_robot_rollout.h, of
    include/salp_robot_sampled.h, of include/salp_robot_evaluate.h, and of every function of include/salp_vec.h and include/salp_robot.h, in header order
    (tests/test_capi_prototypes.py compares the last table with its two headers).  vp: a handle, a buffer (host or device) or a stream."""
    vp, i64, u64, i32, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32
    rc, dbl, ptr = ctypes.c_int, ctypes.c_double, ctypes.POINTER
    create = lambda cfg: (rc, [ptr(cfg), i64, rc, u64, i64, ptr(vp)])
    step = (rc, [vp] * 8 + [u32, vp])                  # h, act, obs, reward, terminated, truncated, final_obs, info / inner_steps
    policy_create = (rc, [vp, ptr(CPolicyDesc), vp, u32, vp, ptr(vp)])
    policy_packed = {     # include/salp_vec_policy_packed.h, in header order (tests/test_capi_policy_packed.py compares it with that header)
        "salp_vec_rollout_policy_packed": (rc, [vp, vp, i32, vp, vp, u32, vp]),
        "salp_vec_rollout_policy_packed_sampled": (rc, [vp, vp, i32, vp, vp, vp, u32, vp]),
    }
    policy_wide = {       # include/salp_vec_policy_wide.h, in header order (tests/test_wide_policy_host.py compares it with that header)
        "salp_policy_words_wide": (rc, [vp, ptr(CPolicyDesc), rc]),
        "salp_policy_create_wide": policy_create,
        "salp_policy_create_gaussian_wide": policy_create,
        "salp_vec_last_launch_policy_wide": (rc, [vp]),
    }
    rollout = {       # include/salp_robot_rollout.h, in header order (tests/test_capi_robot_rollout.py compares it with that header)
        "salp_robot_vec_rollout": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, vp, u32, vp]),
        "salp_robot_policy_words": (rc, [vp, ptr(CPolicyDesc)]),
        "salp_robot_policy_create": policy_create,
        "salp_robot_policy_update": (rc, [vp, vp, u32, vp]),
        "salp_robot_policy_destroy": (None, [vp]),
        "salp_robot_vec_rollout_policy": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, u32, vp]),
    }
    sampled = {       # include/salp_robot_sampled.h, in header order (tests/test_capi_robot_sampled.py compares it with that header)
        "salp_robot_policy_words_gaussian": (rc, [vp, ptr(CPolicyDesc)]),
        "salp_robot_policy_create_gaussian": policy_create,
        "salp_robot_policy_set_noise_step": (rc, [vp, u64, vp]),
        "salp_robot_policy_noise_step": (rc, [vp, ptr(u64)]),
        "salp_robot_vec_rollout_policy_sampled": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]),
    }
    evaluate = {      # include/salp_robot_evaluate.h, in header order (tests/test_capi_robot_evaluate.py compares it with that header)
        "salp_robot_vec_evaluate_policy": (rc, [vp, vp, i32, vp, u32, vp]),
        "salp_robot_vec_evaluate_policy_sampled": (rc, [vp, vp, i32, vp, u32, vp]),
    }
    return policy_packed, policy_wide, rollout, sampled, evaluate, {
        "salp_last_error": (ctypes.c_char_p, []),
        "salp_abi_version": (rc, []),
        "salp_device_count": (rc, []),
        "salp_config_default": (rc, [ptr(CConfig)]),
        "salp_vec_create": create(CConfig),
        "salp_vec_destroy": (None, [vp]),
        "salp_vec_num_envs": (i64, [vp]),
        "salp_vec_obs_dim": (rc, [vp]),
        "salp_vec_act_dim": (rc, [vp]),
        "salp_vec_num_food": (rc, [vp]),
        "salp_vec_device": (rc, [vp]),
        "salp_vec_reset": (rc, [vp, vp, vp, u32, vp]),
        "salp_vec_step": step,
        "salp_vec_rollout": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, vp, u32, vp]),
        "salp_vec_record_width": (rc, [vp, u32]),
        "salp_vec_step_packed": (rc, [vp, vp, vp, u32, vp]),
        "salp_vec_rollout_packed": (rc, [vp, vp, i32, vp, vp, u32, vp]),
        "salp_policy_words": (rc, [vp, ptr(CPolicyDesc)]),
        "salp_policy_create": policy_create,
        "salp_policy_update": (rc, [vp, vp, u32, vp]),
        "salp_policy_destroy": (None, [vp]),
        "salp_policy_words_gaussian": (rc, [vp, ptr(CPolicyDesc)]),
        "salp_policy_create_gaussian": policy_create,
        "salp_policy_set_noise_step": (rc, [vp, u64, vp]),
        "salp_policy_noise_step": (rc, [vp, ptr(u64)]),
        "salp_vec_rollout_policy_sampled": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, vp, u32, vp]),
        "salp_vec_evaluate_policy_sampled": (rc, [vp, vp, i32, vp, u32, vp]),
        "salp_vec_rollout_policy": (rc, [vp, vp, i32, vp, vp, vp, vp, vp, u32, vp]),
        "salp_vec_evaluate_policy": (rc, [vp, vp, i32, vp, u32, vp]),
        "salp_vec_evaluate_navigation": (rc, [vp, vp, i32, vp, dbl, vp, vp, u32, vp]),
        "salp_vec_observe": (rc, [vp, vp, u32, vp]),
        "salp_vec_get_state": (rc, [vp, vp, vp, u32, vp]),
        "salp_vec_set_state": (rc, [vp, vp, vp, u32, vp]),
        "salp_vec_reseed": (rc, [vp, u64, vp, u32, vp]),
        "salp_vec_get_stats": (rc, [vp, ptr(CStats)]),
        "salp_vec_clear_stats": (rc, [vp]),
        "salp_vec_global_step": (i64, [vp]),
        "salp_vec_last_launch": (rc, [vp, ptr(i64)]),
        "salp_vec_last_launch_signatures": (rc, [vp, ptr(i64)]),
        "salp_vec_last_kernel_resources": (rc, [vp, ptr(i32)]),
        "salp_vec_set_base_num_food": (rc, [vp, i32]),
        "salp_vec_base_num_food": (i32, [vp]),
        "salp_robot_last_error": (ctypes.c_char_p, []),
        "salp_robot_config_default": (rc, [ptr(CRobotConfig)]),
        "salp_robot_vec_create": create(CRobotConfig),
        "salp_robot_vec_destroy": (None, [vp]),
        "salp_robot_vec_num_envs": (i64, [vp]),
        "salp_robot_vec_reset": (rc, [vp, vp, vp, u32, vp]),
        "salp_robot_vec_step": step,
        "salp_robot_vec_get_state": (rc, [vp, vp, u32, vp]),
        "salp_robot_vec_history_capacity": (i32, [vp, i32]),
        "salp_robot_vec_step_history": (rc, [vp] * 8 + [i64, i64, i32, i32, vp, vp, u32, vp]),
        "salp_robot_vec_trajectory": (rc, [vp, vp, vp, i32, vp, vp, vp, vp, u32, vp]),
    }


POLICY_PACKED_PROTOTYPES, POLICY_WIDE_PROTOTYPES, ROBOT_ROLLOUT_PROTOTYPES, ROBOT_SAMPLED_PROTOTYPES, ROBOT_EVALUATE_PROTOTYPES, PROTOTYPES = _prototypes()
ROBOT_EXPORTS = tuple(n for n in PROTOTYPES if n.startswith("salp_robot_"))
EXPORTS = tuple(n for n in PROTOTYPES if n not in ROBOT_EXPORTS)

_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Loads libsalp_hip.so and declares every prototype.  Raises SalpError if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SALP_HIP_LIBRARY", LIB_PATH)
    # If PyTorch is installed, let it load ITS HIP runtime first: torch ships its own libamdhip64 and
    # cannot initialise once the system copy (which this library would pull in) is already resident,
    # whereas this library runs on either copy.
    if os.environ.get("SALP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.isfile(p):
        raise SalpError(
            f"HIP library not found at {p}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    L = ctypes.CDLL(p)
    for name, (restype, argtypes) in {**PROTOTYPES, **POLICY_PACKED_PROTOTYPES, **POLICY_WIDE_PROTOTYPES, **ROBOT_ROLLOUT_PROTOTYPES, **ROBOT_SAMPLED_PROTOTYPES,
                                      **ROBOT_EVALUATE_PROTOTYPES}.items():
        # the default library has every symbol (a missing one raises here); an explicit path may be an older A/B
        # variant (profiles/ab_bench.py) that lacks the newer ones
        if path is None or hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    if path is None:
        _lib = L
    return L


def check(lib, rc: int, what: str, last_error: str = "salp_last_error"):
    if rc != 0:
        msg = getattr(lib, last_error)()
        raise SalpError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def address(x):
    """A torch tensor or numpy array as its address; anything else (None, an integer address, a ctypes object) as it is."""
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data if hasattr(x, "ctypes") else x


def call(lib, name: str, *args, what: Optional[str] = None):
    """`name(*args)` of either header, tensors and arrays passed by address; a nonzero status raises SalpError with the
    library's message (`what`: the failing call's name in that message, default `name`)."""
    rc = getattr(lib, name)(*[address(a) for a in args])
    if rc != 0:
        check(lib, rc, what or name, "salp_robot_last_error" if name.startswith("salp_robot_") else "salp_last_error")


class SalpLib:
    """One handle of the C ABI (one GPU).  Pointers are tensors, arrays or raw integers (device or host addresses)."""

    def __init__(self, cfg: SalpSnakeConfig, n_envs: int, device_id: int = 0, seed: int = 0,
                 env_index_base: int = 0):
        self.lib = load_library()
        self.cfg = cfg
        self._c = cfg.to_c()
        self._h = ctypes.c_void_p()
        self._policies = []
        call(self.lib, "salp_vec_create", ctypes.byref(self._c), int(n_envs), int(device_id),
             int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_index_base), ctypes.byref(self._h))
        self.n_envs = int(self.lib.salp_vec_num_envs(self._h))
        self.obs_dim = int(self.lib.salp_vec_obs_dim(self._h))
        self.act_dim = int(self.lib.salp_vec_act_dim(self._h))
        self.num_food = int(self.lib.salp_vec_num_food(self._h))
        self.device_id = int(self.lib.salp_vec_device(self._h))

    def close(self):
        if getattr(self, "_h", None):
            for p in list(self._policies):     # a policy goes before its handle
                p.close()
            self.lib.salp_vec_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _ptr = staticmethod(address)

    def _call(self, name, *args):
        call(self.lib, name, self._h, *args)

    def reset(self, mask, obs, flags, stream=0):
        self._call("salp_vec_reset", mask, obs, flags, stream)

    def step(self, act, obs, reward, term, trunc, final_obs, info, flags, stream=0):
        self._call("salp_vec_step", act, obs, reward, term, trunc, final_obs, info, flags, stream)

    def rollout(self, act, horizon, obs, reward, term, trunc, final_obs, act_out, flags, stream=0):
        self._call("salp_vec_rollout", act, int(horizon), obs, reward, term, trunc, final_obs, act_out, flags, stream)

    def record_width(self, with_final: bool) -> int:
        """Words per packed record of this handle: obs_dim + 4, or 2 obs_dim + 4 with the terminal observation."""
        return int(self.lib.salp_vec_record_width(self._h, REC_FINAL_OBS if with_final else 0))

    def step_packed(self, act, rec, flags, stream=0):
        """salp_vec_step_packed: rec float32 [n, width]; flags: SALP_DEVICE_PTRS and / or REC_FINAL_OBS."""
        self._call("salp_vec_step_packed", act, rec, flags, stream)

    def rollout_packed(self, act, horizon, rec, act_out, flags, stream=0):
        """salp_vec_rollout_packed: rec float32 [horizon, n, width]; act None = device-generated actions (into act_out)."""
        self._call("salp_vec_rollout_packed", act, int(horizon), rec, act_out, flags, stream)

    def policy_words(self, policy) -> int:
        """salp_policy_words: float32 words of one policy of this shape on this handle (raises for a shape out of range)."""
        gauss = bool(getattr(policy, "gaussian", False))
        if getattr(policy, "wide", False):
            name = "salp_policy_words_wide"
            rc = self.lib.salp_policy_words_wide(self._h, ctypes.byref(policy.desc()), int(gauss))
        else:
            name = "salp_policy_words_gaussian" if gauss else "salp_policy_words"
            rc = getattr(self.lib, name)(self._h, ctypes.byref(policy.desc()))
        if rc < 0:
            check(self.lib, rc, name)
        return int(rc)

    def policy_create(self, policy, weights=None, flags=0, stream=0) -> "PolicyHandle":
        """salp_policy_create for an `MLPPolicy` (shape and, unless `weights` is given, its packed float32 weights; `weights`
        with SALP_DEVICE_PTRS: a device block in the public layout [P, words]); salp_policy_create_gaussian for a
        `GaussianPolicy`; the _wide entry points (include/salp_vec_policy_wide.h) for a policy made with `wide=True`."""
        h = ctypes.c_void_p()
        gauss = bool(getattr(policy, "gaussian", False))
        name = ("salp_policy_create_gaussian" if gauss else "salp_policy_create") + ("_wide" if getattr(policy, "wide", False) else "")
        self._call(name, ctypes.byref(policy.desc()),
                   policy.pack() if weights is None else weights, flags, stream, ctypes.byref(h))
        ph = PolicyHandle(self, h, policy.n_policies, int(policy.words), gauss)
        self._policies.append(ph)
        return ph

    def policy_update(self, handle: "PolicyHandle", weights, flags=0, stream=0):
        """salp_policy_update: float32 [P, words] in the public layout; with SALP_DEVICE_PTRS stream-ordered, no allocation."""
        handle.update(weights, flags, stream)

    def rollout_policy(self, handle: "PolicyHandle", horizon, obs, reward, term, trunc, act_out, flags, stream=0):
        """salp_vec_rollout_policy: the four main outputs are required, act_out may be None."""
        self._call("salp_vec_rollout_policy", handle._p, int(horizon), obs, reward, term, trunc, act_out, flags, stream)

    def evaluate_policy(self, handle: "PolicyHandle", horizon, rec, flags, stream=0):
        """salp_vec_evaluate_policy: rec int32 [n, EVAL_WORDS], one summary record per env and nothing per step; flags:
        SALP_DEVICE_PTRS and / or EVAL_ACCUMULATE (continue the records in `rec`)."""
        self._call("salp_vec_evaluate_policy", handle._p, int(horizon), rec, flags, stream)

    def evaluate_navigation(self, handle: "PolicyHandle", horizon, line, goal_radius, rec, track, flags, stream=0):
        """salp_vec_evaluate_navigation: line float64 [n, 4] (start x, y, goal x, y), rec int32 [n, NAV_WORDS], track float64
        [horizon, n, 2] or None; flags: SALP_DEVICE_PTRS and / or EVAL_ACCUMULATE (continue the records in `rec`)."""
        self._call("salp_vec_evaluate_navigation", handle._p, int(horizon), line, float(goal_radius), rec, track, flags, stream)

    def rollout_policy_sampled(self, handle: "PolicyHandle", horizon, obs, reward, term, trunc, act_out, logp_out, flags, stream=0):
        """salp_vec_rollout_policy_sampled: a Gaussian policy's sampled actions; act_out and logp_out may be None."""
        self._call("salp_vec_rollout_policy_sampled", handle._p, int(horizon), obs, reward, term, trunc, act_out, logp_out,
                   flags, stream)

    def rollout_policy_packed(self, handle: "PolicyHandle", horizon, rec, act_out, flags, stream=0):
        """salp_vec_rollout_policy_packed (include/salp_vec_policy_packed.h): the closed loop of rollout_policy writing the
        records of rollout_packed; rec float32 [horizon, n, width], act_out may be None; flags: SALP_DEVICE_PTRS and / or
        REC_FINAL_OBS."""
        self._call("salp_vec_rollout_policy_packed", handle._p, int(horizon), rec, act_out, flags, stream)

    def rollout_policy_packed_sampled(self, handle: "PolicyHandle", horizon, rec, act_out, logp_out, flags, stream=0):
        """salp_vec_rollout_policy_packed_sampled: the same with a Gaussian policy's sampled actions; act_out and logp_out
        may be None."""
        self._call("salp_vec_rollout_policy_packed_sampled", handle._p, int(horizon), rec, act_out, logp_out, flags, stream)

    def evaluate_policy_sampled(self, handle: "PolicyHandle", horizon, rec, flags, stream=0):
        """salp_vec_evaluate_policy_sampled: evaluate_policy under a Gaussian policy's sampled actions."""
        self._call("salp_vec_evaluate_policy_sampled", handle._p, int(horizon), rec, flags, stream)

    def reseed(self, seed, obs, flags, stream=0):
        """New draw streams keyed by `seed`, every env reset from draw counter 0; no reallocation (capture-safe)."""
        self._call("salp_vec_reseed", int(seed) & 0xFFFFFFFFFFFFFFFF, obs, flags, stream)

    def observe(self, obs, flags, stream=0):
        self._call("salp_vec_observe", obs, flags, stream)

    def get_state(self, f64, i32, flags, stream=0):
        self._call("salp_vec_get_state", f64, i32, flags, stream)

    def set_state(self, f64, i32, flags, stream=0):
        self._call("salp_vec_set_state", f64, i32, flags, stream)

    def stats(self) -> dict:
        s = CStats()
        self._call("salp_vec_get_stats", ctypes.byref(s))
        return {k: getattr(s, k) for k, _ in CStats._fields_}

    def last_launch(self) -> dict:
        """The kernel instantiation of the most recent step / rollout call (salp_vec_last_launch).  `full_signature`: 1 = the four
        main outputs only, 2 = the four plus final_obs / info, 3 = the packed record (step_packed / rollout_packed, every
        instantiation; rollout_policy_packed with `actions_in_kernel` 2 or 3), 4 = the per-env summary record and no per-step output (evaluate_policy),
        5 = the navigation record (evaluate_navigation), 0 = every store tested (some main output absent, the generic instantiation, or a predicated launch
        asked for final_obs / info) — of the kernel that ran: the unpredicated launch's
        when there was one, else the predicated launch's.  `signature_unpredicated` / `signature_predicated`: each half's own,
        -1 for a half that was not launched (salp_vec_last_launch_signatures)."""
        a, b = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 2)()
        self._call("salp_vec_last_launch", a)
        self._call("salp_vec_last_launch_signatures", b)
        keys = ("food_slots", "observed_capacity", "literal_constants", "forced", "full_signature", "actions_in_kernel",
                "envs_unpredicated", "envs_predicated", "signature_unpredicated", "signature_predicated")
        return dict(zip(keys, (int(v) for v in (*a, *b))))

    def last_launch_policy_wide(self) -> int:
        """salp_vec_last_launch_policy_wide: 1 when the most recent launch ran the wide policy kernels, else 0."""
        return int(self.lib.salp_vec_last_launch_policy_wide(self._h))

    def last_kernel_resources(self) -> dict:
        """Registers, LDS, scratch and resident workgroups per CU of the most recent call's kernel (salp_vec_last_kernel_resources)."""
        a = (ctypes.c_int32 * 4)()
        self._call("salp_vec_last_kernel_resources", a)
        return dict(zip(("vgprs", "lds_bytes", "scratch_bytes", "workgroups_per_cu"), (int(v) for v in a)))

    def clear_stats(self):
        self._call("salp_vec_clear_stats")

    @property
    def base_num_food(self) -> int:
        return int(self.lib.salp_vec_base_num_food(self._h))

    def set_base_num_food(self, k: int):
        self._call("salp_vec_set_base_num_food", int(k))

    @property
    def global_step(self) -> int:
        return int(self.lib.salp_vec_global_step(self._h))


class PolicyHandleBase:
    """One policy block on a handle's device.  The subclass names its library by the prefix of its functions; `owner` is
    what made the handle: it has the loaded library (`lib`) and lists its live handles (`_policies`)."""
    _prefix = ""
    _what = {}      # function (without the prefix) -> the call's name in an error message, default the function's own

    def __init__(self, owner, p, n_policies: int, words: int, gaussian: bool = False):
        self.owner, self._p, self.n_policies, self.words = owner, p, int(n_policies), int(words)
        self.gaussian = bool(gaussian)

    def _call(self, name, *args):
        call(self.owner.lib, self._prefix + name, self._p, *args, what=self._what.get(name))

    @property
    def noise_step(self) -> int:
        """*_policy_noise_step: the Gaussian policy's noise step (waits for the policy's last stream)."""
        n = ctypes.c_uint64()
        self._call("noise_step", ctypes.byref(n))
        return int(n.value)

    def set_noise_step(self, n: int, stream=0):
        """*_policy_set_noise_step: stream-ordered."""
        self._call("set_noise_step", int(n) & 0xFFFFFFFFFFFFFFFF, stream)

    def update(self, weights, flags=0, stream=0):
        """*_policy_update: float32 [P, words] in the public layout; with SALP_DEVICE_PTRS stream-ordered, no allocation."""
        self._call("update", weights, flags, stream)

    def close(self):
        if getattr(self, "_p", None):
            getattr(self.owner.lib, self._prefix + "destroy")(self._p)
            self._p = ctypes.c_void_p()
            if self in self.owner._policies:
                self.owner._policies.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PolicyHandle(PolicyHandleBase):
    """One salp_policy_t (SalpLib.policy_create)."""
    _prefix = "salp_policy_"
