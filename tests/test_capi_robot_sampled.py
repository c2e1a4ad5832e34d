"""The prototype table `_capi.ROBOT_SAMPLED_PROTOTYPES` against the header it mirrors, include/salp_robot_sampled.h, the way
tests/test_capi_robot_rollout.py holds `_capi.ROBOT_ROLLOUT_PROTOTYPES` to include/salp_robot_rollout.h: every function of
the header is in the table and nothing else is, in header order, with the argument count, each argument's class and the
return type of its declaration; the header is plain C99; the built library exports every name and the loader declares it.
No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import test_capi_prototypes as tp
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.policy import CPolicyDesc

HEADER = "salp_robot_sampled.h"
DECLARED = tp.declarations(HEADER)
NAMES = ("salp_robot_policy_words_gaussian", "salp_robot_policy_create_gaussian", "salp_robot_policy_set_noise_step",
         "salp_robot_policy_noise_step", "salp_robot_vec_rollout_policy_sampled")


def test_the_parser_finds_every_declaration():
    assert tuple(DECLARED) == NAMES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(tp.ROOT, "include", HEADER)).read(), flags=re.S)
    assert set(DECLARED) == {n for n in re.findall(r"\b(salp_[a-z_0-9]+)\s*\(", src) if not n.endswith("_t")}


def test_the_table_has_every_function_in_header_order_and_nothing_else():
    assert tuple(_capi.ROBOT_SAMPLED_PROTOTYPES) == NAMES
    assert not set(_capi.ROBOT_SAMPLED_PROTOTYPES) & (set(_capi.PROTOTYPES) | set(_capi.ROBOT_ROLLOUT_PROTOTYPES))


def test_the_other_robot_headers_gained_no_declaration():
    """The Gaussian calls live in their own header: salp_robot_rollout.h points at it and declares none of them."""
    rollout = open(os.path.join(tp.ROOT, "include", "salp_robot_rollout.h")).read()
    assert "salp_robot_sampled.h" in rollout and "No Gaussian head" not in rollout
    for header in ("salp_robot.h", "salp_robot_rollout.h", "salp_vec.h"):
        assert not set(tp.declarations(header)) & set(NAMES), header


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_its_declaration(name):
    ret, params = DECLARED[name]
    restype, argtypes = _capi.ROBOT_SAMPLED_PROTOTYPES[name]
    assert restype is tp.RETURNS[ret], (name, ret, restype)
    assert len(argtypes) == len(params), (name, params, argtypes)
    for k, (param, ctype) in enumerate(zip(params, argtypes)):
        if "*" in param:
            assert tp.is_pointer(ctype), (name, k, param, ctype)
            if re.search(r"\bsalp_policy_desc_t\s*\*", param):
                assert ctype._type_ is CPolicyDesc, (name, param)
            if re.search(r"\buint64_t\s*\*", param):
                assert ctype._type_ is ctypes.c_uint64, (name, param)
        else:
            words = [w for w in param.split() if w != "const"]
            assert len(words) == 2 and ctype is tp.SCALARS[words[0]], (name, k, param, ctype)


def test_the_sampled_call_is_its_deterministic_twin_plus_logp_out():
    twin = tp.declarations("salp_robot_rollout.h")["salp_robot_vec_rollout_policy"]
    ret, params = DECLARED["salp_robot_vec_rollout_policy_sampled"]
    assert ret == twin[0]
    k = twin[1].index("float* act_out")
    assert params == twin[1][:k + 1] + ["float* logp_out"] + twin[1][k + 1:]


def test_the_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "hdr.c"
    src.write_text(f'#include "{HEADER}"\n'
                   "int main(void) { salp_policy_desc_t d; salp_robot_policy_t* p = 0; uint64_t n = 0;\n"
                   "  int (*get)(salp_robot_policy_t*, uint64_t*) = salp_robot_policy_noise_step; (void)d; (void)p; (void)n; (void)get;\n"
                   "  return SALP_ROBOT_MAX_ROLLOUT_CYCLES == 1024 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(tp.ROOT, "include"),
                    "-fsyntax-only", str(src)], check=True)


def test_the_library_exports_and_the_loader_declares_every_function():
    lib = _capi.load_library()
    for name, (restype, argtypes) in _capi.ROBOT_SAMPLED_PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    raw = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(raw, n) for n in NAMES)
