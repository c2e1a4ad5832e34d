"""The prototype table `_capi.POLICY_PACKED_PROTOTYPES` against the header it mirrors, include/salp_vec_policy_packed.h, the
way tests/test_capi_robot_rollout.py holds `_capi.ROBOT_ROLLOUT_PROTOTYPES` to include/salp_robot_rollout.h: every function of
the header is in the table and nothing else is, in header order, with the argument count, each argument's class and the
return type of its declaration; each call is its parent in salp_vec.h with the record in place of the four streams; the
header is plain C99; the built library exports every name and the loader declares it; and a call that cannot run (no
handle, which is all there is without a GPU) fails with a status and a message.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import test_capi_prototypes as tp
from underwater_swimmer_rl_amd import _capi

HEADER = "salp_vec_policy_packed.h"
DECLARED = tp.declarations(HEADER)
NAMES = ("salp_vec_rollout_policy_packed", "salp_vec_rollout_policy_packed_sampled")


def test_the_parser_finds_every_declaration():
    assert tuple(DECLARED) == NAMES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(tp.ROOT, "include", HEADER)).read(), flags=re.S)
    assert set(DECLARED) == {n for n in re.findall(r"\b(salp_[a-z_0-9]+)\s*\(", src) if not n.endswith("_t")}
    assert '#include "salp_vec.h"' in src


def test_the_table_has_every_function_in_header_order_and_nothing_else():
    assert tuple(_capi.POLICY_PACKED_PROTOTYPES) == NAMES
    others = (set(_capi.PROTOTYPES) | set(_capi.ROBOT_ROLLOUT_PROTOTYPES) | set(_capi.ROBOT_SAMPLED_PROTOTYPES)
              | set(_capi.ROBOT_EVALUATE_PROTOTYPES))
    assert not set(_capi.POLICY_PACKED_PROTOTYPES) & others
    assert not set(NAMES) & set(_capi.EXPORTS)        # EXPORTS stays the list of salp_vec.h


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_its_declaration(name):
    ret, params = DECLARED[name]
    restype, argtypes = _capi.POLICY_PACKED_PROTOTYPES[name]
    assert restype is tp.RETURNS[ret], (name, ret, restype)
    assert len(argtypes) == len(params), (name, params, argtypes)
    for k, (param, ctype) in enumerate(zip(params, argtypes)):
        if "*" in param:
            assert tp.is_pointer(ctype), (name, k, param, ctype)
        else:
            words = [w for w in param.split() if w != "const"]
            assert len(words) == 2 and ctype is tp.SCALARS[words[0]], (name, k, param, ctype)


def test_each_call_is_its_parent_with_the_record_for_the_four_streams():
    """(h, pol, horizon, <outputs>, act_out[, logp_out], flags, stream): the outputs of salp_vec_rollout_policy(_sampled) are
    obs, reward, terminated, truncated; here they are `float* rec`, as in salp_vec_rollout_packed."""
    streams = ["float* obs", "float* reward", "uint8_t* terminated", "uint8_t* truncated"]
    assert "float* rec" in tp.SNAKE["salp_vec_rollout_packed"][1]
    for name, parent in (("salp_vec_rollout_policy_packed", "salp_vec_rollout_policy"),
                         ("salp_vec_rollout_policy_packed_sampled", "salp_vec_rollout_policy_sampled")):
        ret, params = tp.SNAKE[parent]
        k = params.index(streams[0])
        assert params[k:k + 4] == streams
        assert DECLARED[name] == (ret, params[:k] + ["float* rec"] + params[k + 4:]), name
    plain, sampled = (DECLARED[n][1] for n in NAMES)
    k = plain.index("float* act_out")
    assert sampled == plain[:k + 1] + ["float* logp_out"] + plain[k + 1:]


def test_the_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "hdr.c"
    src.write_text(f'#include "{HEADER}"\n'
                   "int main(void) {\n"
                   "  int (*a)(salp_vec_t*, const salp_policy_t*, int32_t, float*, float*, uint32_t, void*) = salp_vec_rollout_policy_packed;\n"
                   "  int (*b)(salp_vec_t*, const salp_policy_t*, int32_t, float*, float*, float*, uint32_t, void*) = salp_vec_rollout_policy_packed_sampled;\n"
                   "  (void)a; (void)b;\n"
                   "  return (SALP_DEVICE_PTRS | SALP_REC_FINAL_OBS) == 3 && SALP_REC_EXTRA_COLS == 4 ? 0 : 1; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(tp.ROOT, "include"),
                    "-fsyntax-only", str(src)], check=True)


def test_the_library_exports_and_the_loader_declares_every_function():
    lib = _capi.load_library()
    for name, (restype, argtypes) in _capi.POLICY_PACKED_PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    raw = ctypes.CDLL(_capi.LIB_PATH)
    assert all(hasattr(raw, n) for n in NAMES)


def test_a_call_without_a_handle_fails_with_a_status_and_a_message():
    """All there is to call without a GPU (salp_vec_create needs one): no handle, no policy.  SALP_ERR_INVALID and a
    message; nothing is read through any pointer, so nothing can crash."""
    lib = _capi.load_library()
    rec = (ctypes.c_float * 64)()
    addr = ctypes.addressof(rec)
    for flags in (0, _capi.REC_FINAL_OBS, _capi.SALP_DEVICE_PTRS | _capi.REC_FINAL_OBS, 8):
        assert lib.salp_vec_rollout_policy_packed(None, None, 4, addr, None, flags, None) == -1
        assert b"NULL" in lib.salp_last_error()
        assert lib.salp_vec_rollout_policy_packed_sampled(None, None, 4, addr, None, None, flags, None) == -1
        assert b"NULL" in lib.salp_last_error()
    assert not any(rec)
