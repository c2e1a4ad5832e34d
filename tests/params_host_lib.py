"""ctypes bindings of the snake simulator's parameter derivation on the host — TEST INFRASTRUCTURE.

oracle/libsalp_params_host.so is tests/params_host.cpp: csrc/salp_params.h compiled as plain C++.  What salp_vec_create
runs before it touches a GPU is callable here without one: default_config(), validate(), make_params(), is_std(), and
the list of literal constants (SALP_STD_CONSTS) that StdConsts and is_std() are generated from.
"""
import ctypes
import os
import re

import native_lib
from native_lib import cint, dbl, i64, ptr, text, u64, vp
from underwater_swimmer_rl_amd.config import CConfig

_II = os.path.join(native_lib.ORACLE_DIR, "salp_params_host.ii")     # made with the library


# every function tests/params_host.cpp exports, in its order
PROTOTYPES = {
    "salp_params_host_default": (None, [ptr(CConfig)]),
    "salp_params_host_validate": (cint, [ptr(CConfig), ptr(text)]),
    "salp_params_host_sizeof": (cint, []),
    "salp_params_host_make": (None, [ptr(CConfig), i64, i64, u64, i64, vp]),
    "salp_params_host_is_std": (cint, [vp]),
    "salp_params_host_const_count": (cint, []),
    "salp_params_host_const_type": (text, [cint]),
    "salp_params_host_const_name": (text, [cint]),
    "salp_params_host_const_text": (text, [cint]),
    "salp_params_host_const_literal": (dbl, [cint]),
    "salp_params_host_const_value": (dbl, [vp, cint]),
}


def lib():
    return native_lib.load("libsalp_params_host.so", PROTOTYPES)


def default_config() -> CConfig:
    c = CConfig()
    lib().salp_params_host_default(ctypes.byref(c))
    return c


def changed(cfg: CConfig, **fields) -> CConfig:
    """A copy of `cfg` with the given fields set."""
    c = CConfig.from_buffer_copy(cfg)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def validate(cfg):
    """(status, message) of validate(); cfg None is the NULL config."""
    why = ctypes.c_char_p()
    rc = lib().salp_params_host_validate(None if cfg is None else ctypes.byref(cfg), ctypes.byref(why))
    return rc, why.value.decode()


class Params:
    """The DevParams that make_params() derives from `cfg`, as an opaque block."""

    def __init__(self, cfg: CConfig, n=64, pitch=64, seed=0, base=0):
        self.buf = ctypes.create_string_buffer(lib().salp_params_host_sizeof())
        lib().salp_params_host_make(ctypes.byref(cfg), n, pitch, seed, base, self.buf)

    def is_std(self) -> bool:
        return bool(lib().salp_params_host_is_std(self.buf))

    def value(self, i: int) -> float:
        """The field that row i of the list names, widened to double (exact for float and int)."""
        return lib().salp_params_host_const_value(self.buf, i)


def std_consts():
    """Rows of SALP_STD_CONSTS: (type, name, literal as written, its value widened to double)."""
    L = lib()
    return [(L.salp_params_host_const_type(i).decode(), L.salp_params_host_const_name(i).decode(),
             L.salp_params_host_const_text(i).decode(), L.salp_params_host_const_literal(i))
            for i in range(L.salp_params_host_const_count())]


def std_members_after_preprocessing():
    """The `static constexpr` member names of struct StdConsts as the compiler sees them (oracle/salp_params_host.ii)."""
    lib()
    with open(_II) as f:
        body = re.search(r"struct StdConsts \{(.*?)\};", f.read(), re.S).group(1)
    return re.findall(r"static constexpr \w+ (\w+) =", body)
