"""The prototype table `_capi.ROBOT_EVALUATE_PROTOTYPES` against the header it mirrors, include/salp_robot_evaluate.h, the
way tests/test_capi_robot_sampled.py holds `_capi.ROBOT_SAMPLED_PROTOTYPES` to include/salp_robot_sampled.h: every function
of the header is in the table and nothing else is, in header order, with the argument count, each argument's class and the
return type of its declaration; the other headers declare neither; the header is plain C99 with the record's constants;
the built library exports every name and the loader declares it.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import test_capi_prototypes as tp
from underwater_swimmer_rl_amd import _capi, policy

HEADER = "salp_robot_evaluate.h"
DECLARED = tp.declarations(HEADER)
NAMES = ("salp_robot_vec_evaluate_policy", "salp_robot_vec_evaluate_policy_sampled")


def test_the_parser_finds_every_declaration():
    assert tuple(DECLARED) == NAMES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(tp.ROOT, "include", HEADER)).read(), flags=re.S)
    assert set(DECLARED) == {n for n in re.findall(r"\b(salp_[a-z_0-9]+)\s*\(", src) if not n.endswith("_t")}


def test_the_table_has_every_function_in_header_order_and_nothing_else():
    assert tuple(_capi.ROBOT_EVALUATE_PROTOTYPES) == NAMES
    others = set(_capi.PROTOTYPES) | set(_capi.ROBOT_ROLLOUT_PROTOTYPES) | set(_capi.ROBOT_SAMPLED_PROTOTYPES)
    assert not set(_capi.ROBOT_EVALUATE_PROTOTYPES) & others
    assert not set(NAMES) & set(_capi.ROBOT_EXPORTS)


def test_the_other_headers_gained_no_declaration():
    for header in ("salp_robot.h", "salp_robot_rollout.h", "salp_robot_sampled.h", "salp_vec.h"):
        assert not set(tp.declarations(header)) & set(NAMES), header


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_its_declaration(name):
    ret, params = DECLARED[name]
    restype, argtypes = _capi.ROBOT_EVALUATE_PROTOTYPES[name]
    assert restype is tp.RETURNS[ret], (name, ret, restype)
    assert len(argtypes) == len(params), (name, params, argtypes)
    for k, (param, ctype) in enumerate(zip(params, argtypes)):
        if "*" in param:
            assert tp.is_pointer(ctype), (name, k, param, ctype)
        else:
            words = [w for w in param.split() if w != "const"]
            assert len(words) == 2 and ctype is tp.SCALARS[words[0]], (name, k, param, ctype)


def test_the_two_calls_take_the_same_arguments():
    assert DECLARED[NAMES[0]] == DECLARED[NAMES[1]]
    assert DECLARED[NAMES[0]][1] == ["salp_robot_vec_t* h", "const salp_robot_policy_t* pol", "int32_t horizon", "void* rec",
                                     "uint32_t flags", "void* stream"]


def test_the_header_is_plain_c99_and_states_the_record(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    fields = {"RETURN": policy.REVAL_RETURN, "FIRST_RETURN": policy.REVAL_FIRST_RETURN, "EULER_STEPS": policy.REVAL_EULER_STEPS,
              "FIRST_LENGTH": policy.REVAL_FIRST_LENGTH, "FIRST_END": policy.REVAL_FIRST_END, "EPISODES": policy.REVAL_EPISODES,
              "REACHED": policy.REVAL_REACHED, "FIRST_EULER_STEPS": policy.REVAL_FIRST_EULER_STEPS, "WORDS": policy.REVAL_WORDS}
    checks = "".join(f"typedef char reval_{k.lower()}[SALP_REVAL_{k} == {v} ? 1 : -1];\n" for k, v in fields.items())
    src = tmp_path / "hdr.c"
    src.write_text(f'#include "{HEADER}"\n' + checks +
                   "typedef char words_are_12[SALP_REVAL_WORDS == 12 ? 1 : -1];\n"
                   f"typedef char acc[SALP_ROBOT_EVAL_ACCUMULATE == {policy.REVAL_ACCUMULATE} && (int)SALP_ROBOT_EVAL_ACCUMULATE == (int)SALP_EVAL_ACCUMULATE ? 1 : -1];\n"
                   f"typedef char first[SALP_ROBOT_EVAL_FIRST_EPISODE == {policy.REVAL_FIRST_EPISODE} ? 1 : -1];\n"
                   "int main(void) { salp_robot_policy_t* p = 0;\n"
                   "  int (*f)(salp_robot_vec_t*, const salp_robot_policy_t*, int32_t, void*, uint32_t, void*) = salp_robot_vec_evaluate_policy;\n"
                   "  f = salp_robot_vec_evaluate_policy_sampled; (void)p; (void)f;\n"
                   "  return SALP_ROBOT_MAX_ROLLOUT_CYCLES == 1024 && SALP_DEVICE_PTRS == 1 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(tp.ROOT, "include"),
                    "-fsyntax-only", str(src)], check=True)


def test_the_library_exports_and_the_loader_declares_every_function():
    lib = _capi.load_library()
    for name, (restype, argtypes) in _capi.ROBOT_EVALUATE_PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    raw = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(raw, n) for n in NAMES)
