"""The C-ABI library loads and exports every symbol include/salp_vec.h declares (no compute
calls: this runs without a GPU), and it fails loudly instead of falling back to a CPU path."""
import ctypes
import os
import re

import pytest

import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.config import CConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "salp_vec.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(salp_[a-z_0-9]+)\s*\(", src)
    return sorted(set(n for n in names if not n.endswith("_t")))


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_salp_build", os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    return _capi.load_library()


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/salp_vec.h but not exported"
    assert set(_capi.EXPORTS) == set(names)


def test_abi_version_and_config_layout(lib):
    assert lib.salp_abi_version() == 1
    c = CConfig()
    assert lib.salp_config_default(ctypes.byref(c)) == 0
    assert c.struct_size == ctypes.sizeof(CConfig)
    d = pkg.SalpSnakeConfig()          # python defaults == C defaults == snake:29-33 / legacy:32-53
    e = d.to_c()
    for name, _ in CConfig._fields_:
        assert getattr(c, name) == getattr(e, name), name


def test_no_cpu_fallback(lib):
    """Without a HIP device create() must fail with SALP_ERR_NO_DEVICE, never simulate on the CPU."""
    if lib.salp_device_count() > 0:
        pytest.skip("a GPU is visible here")
    c = pkg.load_env_config("single_food").to_c()
    h = ctypes.c_void_p()
    rc = lib.salp_vec_create(ctypes.byref(c), 64, 0, 0, 0, ctypes.byref(h))
    assert rc == -2 and not h
    assert b"no HIP device" in lib.salp_last_error()
    with pytest.raises(_capi.SalpError):
        pkg.SalpVectorEnv("single_food", 64, output="numpy")


def test_bad_config_is_rejected_before_touching_the_device(lib):
    c = pkg.load_env_config("single_food").to_c()
    h = ctypes.c_void_p()
    c.struct_size = 4
    assert lib.salp_vec_create(ctypes.byref(c), 64, 0, 0, 0, ctypes.byref(h)) == -1
    c = pkg.load_env_config("single_food").to_c()
    c.num_food_items = 99
    assert lib.salp_vec_create(ctypes.byref(c), 64, 0, 0, 0, ctypes.byref(h)) == -1
    assert lib.salp_vec_create(None, 64, 0, 0, 0, ctypes.byref(h)) == -1
    assert lib.salp_vec_num_envs(None) == 0 and lib.salp_vec_obs_dim(None) == 0
    lib.salp_vec_destroy(None)  # no-op


def test_missing_library_raises(tmp_path):
    with pytest.raises(_capi.SalpError):
        _capi.load_library(str(tmp_path / "nope.so"))


def test_robot_abi_symbols_are_exported(lib):
    """include/salp_robot.h (HEAD simulator)."""
    from underwater_swimmer_rl_amd.robot_env import ROBOT_EXPORTS, CRobotConfig
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "salp_robot.h")).read(), flags=re.S)
    names = sorted(set(n for n in re.findall(r"\b(salp_robot_[a-z_0-9]+)\s*\(", src) if not n.endswith("_t")))
    assert set(names) == set(ROBOT_EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    c = CRobotConfig()
    lib.salp_robot_config_default.argtypes = [ctypes.POINTER(CRobotConfig)]
    assert lib.salp_robot_config_default(ctypes.byref(c)) == 0 and c.struct_size == ctypes.sizeof(CRobotConfig)
    assert (c.width, c.height, c.max_cycles, c.dt, c.nozzle_area) == (900, 700, 500, 0.01, 0.00016)


def test_headers_are_plain_c99(tmp_path):
    """The boundary is a C ABI: both headers must compile as C99 (no C++, no torch types)."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "hdr.c"
    src.write_text('#include "salp_vec.h"\n#include "salp_robot.h"\n'
                   "int main(void) { salp_config_t c; salp_robot_config_t r; salp_stats_t s; (void)c; (void)r; (void)s; return 0; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    "-fsyntax-only", str(src)], check=True)


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_salp_build", os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


ROLLOUT_K3_UNITS = {f"salp_rollout_f{slots}_{consts}.hip" for slots in (1, 4, 8, 12, 16) for consts in ("std", "rt")}


def test_build_compiles_every_hip_source():
    """csrc/build.py compiles what is there: its source list is the csrc/*.hip glob, the rollout kernel units among them."""
    import glob
    b = _build_module()
    csrc = os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc")
    assert sorted(os.path.realpath(s) for s in b.sources()) == sorted(os.path.realpath(s) for s in glob.glob(os.path.join(csrc, "*.hip")))
    assert {os.path.basename(s) for s in b.sources()} == {"salp_vec.hip", "salp_robot.hip", "salp_rollout_generic.hip"} | ROLLOUT_K3_UNITS


def test_rollout_units_are_compiled_without_machine_licm():
    """-mllvm -disable-machine-licm (csrc/build.py on why) goes to every rollout kernel unit and to salp_vec.hip, not to
    salp_robot.hip; and never more than 16 compilers run at once."""
    b = _build_module()
    flags = {os.path.basename(s): f for s, f in b.SRC_FLAGS.items()}
    assert set(flags) == {os.path.basename(s) for s in b.sources()}
    for name, f in flags.items():
        assert (" ".join(f) == "-mllvm -disable-machine-licm") == (name != "salp_robot.hip"), (name, f)
    assert sum(n.startswith("salp_rollout_") for n in flags) == 11
    old = os.environ.get("MAX_JOBS")
    try:
        for given, want in (("3", 3), ("64", 16), ("0", 1)):
            os.environ["MAX_JOBS"] = given
            assert b.max_jobs() == want
        del os.environ["MAX_JOBS"]
        assert 1 <= b.max_jobs() <= 16
    finally:
        if old is not None:
            os.environ["MAX_JOBS"] = old


STAND_IN_COMPILER = """#!/bin/sh
# stands for hipcc: fails at once for sources whose path contains $STAND_IN_FAIL, else writes the object and stays
echo "$$" >> "$STAND_IN_PIDS"
while [ $# -gt 1 ]; do [ "$1" = "-o" ] && obj=$2; shift; done
case "$1" in *"$STAND_IN_FAIL"*) exit 1;; esac
: > "$obj"
sleep 600 &
echo "$!" >> "$STAND_IN_PIDS"
wait
"""


def _alive(pid):
    try:
        with open(f"/proc/{pid}/stat") as f:
            return f.read().rsplit(")", 1)[1].split()[0] != "Z"
    except OSError:
        return False


@pytest.mark.parametrize("fail, started", [("salp_robot.hip", 8), (".hip", 8)])
def test_a_failed_compile_raises_and_leaves_nothing_behind(tmp_path, monkeypatch, fail, started):
    """One compiler fails while seven others run (salp_robot.hip is the first source), or all eight fail in the same
    instant (an error in the shared header): build() raises the compiler's CalledProcessError, starts no further
    compiler, leaves no compiler or child of one running and no object file."""
    import glob
    import subprocess
    import time
    cc, pids = tmp_path / "hipcc", tmp_path / "pids"
    cc.write_text(STAND_IN_COMPILER)
    cc.chmod(0o755)
    for k, v in (("HIPCC", str(cc)), ("MAX_JOBS", "8"), ("STAND_IN_FAIL", fail), ("STAND_IN_PIDS", str(pids))):
        monkeypatch.setenv(k, v)
    b = _build_module()
    out = str(tmp_path / "lib.so")
    with pytest.raises(subprocess.CalledProcessError) as e:
        b.build(force=True, out=out)
    assert e.value.returncode == 1 and e.value.cmd[0] == str(cc)
    assert glob.glob(str(tmp_path / "*.o")) == [] and not os.path.exists(out) and not os.path.exists(out + ".hash")
    seen = [int(x) for x in pids.read_text().split()]
    assert len(seen) == started + (7 if fail == "salp_robot.hip" else 0)      # the stand-ins and the sleeping children
    deadline = time.monotonic() + 5.0          # a signalled child may take a moment to go
    while any(_alive(p) for p in seen) and time.monotonic() < deadline:
        time.sleep(0.01)
    assert [p for p in seen if _alive(p)] == []


def test_build_dependencies_cover_every_source_file(lib):
    """The staleness check of csrc/build.py: every header / source the library is compiled from is a dependency (globbed),
    and an edit to any ONE of them — content, not file time — makes the built library stale.  (Round 2 shipped a
    hand-written list that missed salp_food_reg.h, and prebuilt .so files travel to the GPU box.)"""
    import glob
    import shutil
    import tempfile
    b = _build_module()
    deps = b.deps()
    csrc = os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc")
    want = glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    assert sorted(os.path.realpath(d) for d in deps) == sorted(os.path.realpath(w) for w in want)
    names = {os.path.basename(d) for d in deps}
    assert {"salp_vec.hip", "salp_robot.hip", "salp_device.h", "salp_food_lds.h", "salp_food_reg.h", "salp_vec.h", "salp_robot.h",
            "salp_rollout_kernel.h", "salp_rollout_generic.hip"} | ROLLOUT_K3_UNITS <= names
    assert b.is_current()                       # the fixture built it: the stored hash matches the tree
    # touch every dependency in turn (in a scratch copy of the tree) and see the library go stale
    with tempfile.TemporaryDirectory() as tmp:
        copies = []
        for d in deps:
            c = os.path.join(tmp, os.path.basename(d))
            shutil.copy(d, c)
            copies.append(c)
        real_deps, b.deps = b.deps, (lambda: sorted(copies))
        try:
            base = b.source_hash()
            out = os.path.join(tmp, "lib.so")
            open(out, "wb").close()
            with open(out + ".hash", "w") as f:
                f.write(base + "\n")
            assert b.is_current(out)
            for c in copies:
                with open(c, "ab") as f:
                    f.write(b"\n// touched\n")
                assert b.source_hash() != base, c
                assert not b.is_current(out), c     # build() would recompile
                shutil.copy([d for d in deps if os.path.basename(d) == os.path.basename(c)][0], c)
                assert b.is_current(out)
            assert not b.is_current(out, defines=("SALP_EXP_STAMPS",))   # another variant is another library
        finally:
            b.deps = real_deps
