"""The one loader of the native test libraries of oracle/ — TEST INFRASTRUCTURE.

oracle/Makefile holds the recipe and knows the dependencies (the compiler writes them), and it replaces a library
atomically, so the rule here is: always ask make.  Up to date, that takes milliseconds.  A prototype table is
name -> (restype, argtypes), in the shape of _capi.PROTOTYPES; tests/test_native_lib.py holds each table to what its
library exports.
"""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
# the names the prototype tables are written in (vp: a handle or a buffer; text: a C string)
vp, cint, i32, u32, i64, u64, dbl, text, ptr = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64,
                                                ctypes.c_uint64, ctypes.c_double, ctypes.c_char_p, ctypes.POINTER)

_libs = {}


def make(target: str) -> str:
    """Brings oracle/<target> up to date; its path."""
    subprocess.run(["make", "-C", ORACLE_DIR, "-s", target], check=True)
    return os.path.join(ORACLE_DIR, target)


def declare(L: ctypes.CDLL, prototypes: dict) -> ctypes.CDLL:
    for name, (restype, argtypes) in prototypes.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def load(target: str, prototypes: dict) -> ctypes.CDLL:
    """oracle/<target>, up to date, with every prototype of the table declared; one CDLL per process and target."""
    if target not in _libs:
        _libs[target] = declare(ctypes.CDLL(make(target)), prototypes)
    return _libs[target]
