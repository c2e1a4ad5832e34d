"""profiles/isa_kernel_diff.py --modulo-registers on tiny synthetic dumps: what counts as the same kernel.

(a) identical bodies;  (b) identical multisets of instructions with every register operand replaced by its class and width.
The .amdhsa_kernel descriptor is compared exactly in both."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "profiles", "isa_kernel_diff.py")

DUMP = """\t.text
\t.globl\tkern
kern:                                   ; @kern
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_lshlrev_b32_e32 v1, 2, v0
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dword v2, v1, s[0:1]
\tv_accvgpr_write_b32 a0, v2
\ts_waitcnt vmcnt(0)
\tv_add_f32_e32 v2, 1.0, v2
\tglobal_store_dword v1, v2, s[0:1]
\ts_endpgm
.Lfunc_end0:
\t.amdhsa_kernel kern
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 3
\t\t.amdhsa_next_free_sgpr 6
\t\t.amdhsa_accum_offset 4
\t.end_amdhsa_kernel
"""


def tool():
    spec = importlib.util.spec_from_file_location("isa_kernel_diff", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def verdicts(tmp_path, new_text):
    """((a) identical, (b) identical modulo registers and order, the tool's exit status in each mode)."""
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(DUMP)
    new.write_text(new_text)
    m = tool()
    (ko, _), (kn, _) = m.kernels(str(old)), m.kernels(str(new))
    assert list(ko) == list(kn) == ["kern"]
    a = ko["kern"] == kn["kern"]
    b = a or m.same_modulo_registers(ko["kern"], kn["kern"])
    plain = subprocess.run([sys.executable, TOOL, str(old), str(new)], capture_output=True, text=True)
    modulo = subprocess.run([sys.executable, TOOL, "--modulo-registers", str(old), str(new)], capture_output=True, text=True)
    return a, b, plain.returncode, modulo.returncode, modulo.stdout


def test_the_same_dump_is_identical_under_both(tmp_path):
    a, b, plain, modulo, out = verdicts(tmp_path, DUMP.replace("; @kern", "; another comment"))
    assert (a, b, plain, modulo) == (True, True, 0, 0)
    assert "identical (a): 1 of 1" in out and "(b): 1 of 1" in out


def test_renamed_and_reordered_registers_are_equal_under_b_only(tmp_path):
    new = DUMP.replace("v2", "v7").replace("s[0:1]", "s[2:3]").replace("a0", "a3")
    lines = new.split("\n")
    i, j = lines.index("\tv_lshlrev_b32_e32 v1, 2, v0"), lines.index("\ts_waitcnt lgkmcnt(0)")
    lines[i], lines[j] = lines[j], lines[i]                       # the same instructions in another order
    a, b, plain, modulo, out = verdicts(tmp_path, "\n".join(lines))
    assert (a, b) == (False, True)
    assert plain == 1 and modulo == 0
    assert "reordered: kern" in out and "identical (a): 0 of 1" in out and "(b): 1 of 1" in out


def test_a_register_of_another_width_or_class_differs_under_both(tmp_path):
    for old, new in (("global_load_dword v2, v1, s[0:1]", "global_load_dword v2, v1, s[0:3]"),
                     ("v_accvgpr_write_b32 a0, v2", "v_accvgpr_write_b32 a0, s2")):
        a, b, plain, modulo, _ = verdicts(tmp_path, DUMP.replace(old, new))
        assert (a, b, plain, modulo) == (False, False, 1, 1), (old, new)


def test_a_changed_opcode_differs_under_both(tmp_path):
    a, b, plain, modulo, out = verdicts(tmp_path, DUMP.replace("v_add_f32_e32 v2, 1.0, v2", "v_mul_f32_e32 v2, 1.0, v2"))
    assert (a, b, plain, modulo) == (False, False, 1, 1)
    assert "differs: kern" in out


def test_a_changed_immediate_differs_under_both(tmp_path):
    a, b, plain, modulo, _ = verdicts(tmp_path, DUMP.replace("v_lshlrev_b32_e32 v1, 2, v0", "v_lshlrev_b32_e32 v1, 3, v0"))
    assert (a, b, plain, modulo) == (False, False, 1, 1)


def test_a_changed_next_free_vgpr_differs_under_both(tmp_path):
    a, b, plain, modulo, out = verdicts(tmp_path, DUMP.replace(".amdhsa_next_free_vgpr 3", ".amdhsa_next_free_vgpr 5"))
    assert (a, b, plain, modulo) == (False, False, 1, 1)
    assert "differs: kern" in out
