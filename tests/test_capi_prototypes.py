"""The prototype table of _capi.py against the two headers it mirrors: every function of include/salp_vec.h and
include/salp_robot.h is in `_capi.PROTOTYPES` and nothing else is, with the argument count, each argument's class
(pointer / the fixed-width integer / double) and the return type of its declaration.  No GPU and no library needed."""
import ctypes
import os
import re

import pytest

from underwater_swimmer_rl_amd import _capi, robot_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "int": ctypes.c_int, "double": ctypes.c_double}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "const char*": ctypes.c_char_p,
           "void": None}


def declarations(header):
    """name -> (return type, [parameter text]) of every `ret name(args);` of the header, comments stripped."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(salp_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = " ".join(args.split())
        out[name] = (re.sub(r"\s*\*", "*", ret.strip()), [] if args == "void" else [a.strip() for a in args.split(",")])
    return out


SNAKE, ROBOT = declarations("salp_vec.h"), declarations("salp_robot.h")
DECLARED = {**SNAKE, **ROBOT}


def is_pointer(ctype):
    return ctype is ctypes.c_void_p or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))


def test_the_parser_finds_every_declaration():
    assert (len(SNAKE), len(ROBOT)) == (42, 11) and not set(SNAKE) & set(ROBOT)
    # the looser search of test_capi_library.py (any `salp_x(` outside a comment) finds the same names
    for header, found in (("salp_vec.h", SNAKE), ("salp_robot.h", ROBOT)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert set(found) == {n for n in re.findall(r"\b(salp_[a-z_0-9]+)\s*\(", src) if not n.endswith("_t")}


def test_the_table_has_every_function_and_nothing_else():
    assert set(_capi.PROTOTYPES) == set(DECLARED)
    assert set(_capi.EXPORTS) == set(SNAKE) and set(_capi.ROBOT_EXPORTS) == set(ROBOT)
    assert robot_env.ROBOT_EXPORTS is _capi.ROBOT_EXPORTS and robot_env.CRobotConfig is _capi.CRobotConfig


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_prototype_matches_its_declaration(name):
    ret, params = DECLARED[name]
    restype, argtypes = _capi.PROTOTYPES[name]
    assert ret in RETURNS, ret
    assert restype is RETURNS[ret], (name, ret, restype)
    assert len(argtypes) == len(params), (name, params, argtypes)
    for k, (param, ctype) in enumerate(zip(params, argtypes)):
        if "*" in param or param.endswith("]"):            # `int64_t info[8]` is a pointer parameter too
            assert is_pointer(ctype), (name, k, param, ctype)
        else:
            words = [w for w in param.split() if w != "const"]
            assert len(words) == 2 and words[0] in SCALARS, (name, k, param)
            assert ctype is SCALARS[words[0]], (name, k, param, ctype)


def test_pointer_parameters_of_a_struct_use_that_struct():
    """Where the table names a struct, it is the one of that parameter's type."""
    from underwater_swimmer_rl_amd.config import CConfig
    from underwater_swimmer_rl_amd.policy import CPolicyDesc
    structs = {"salp_config_t": CConfig, "salp_robot_config_t": _capi.CRobotConfig, "salp_policy_desc_t": CPolicyDesc,
               "salp_stats_t": _capi.CStats}
    seen = set()
    for name, (_, params) in DECLARED.items():
        for param, ctype in zip(params, _capi.PROTOTYPES[name][1]):
            for cname, struct in structs.items():
                if re.search(rf"\b{cname}\s*\*", param):
                    assert ctype._type_ is struct, (name, param, ctype)
                    seen.add(cname)
    assert seen == set(structs)
