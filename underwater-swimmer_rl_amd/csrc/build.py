"""Builds libsalp_hip.so (gfx950) in-tree with hipcc.  `python build.py [--force]`."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "salp_vec.hip")             # the C ABI of SalpSnakeEnv.step's hot path: host code; the service kernels it compiles are salp_service_kernels.h
SRC_ROBOT = os.path.join(HERE, "salp_robot.hip")     # the C ABI of the HEAD Robot simulator: host code; its kernels are salp_robot_kernels.h
INCLUDE = os.path.normpath(os.path.join(HERE, "..", "..", "include"))


def deps() -> list:
    """Every file the library is compiled from: all of csrc/*.h, csrc/*.hip and include/*.h (globbed, so that a new
    header cannot be forgotten — round 2 shipped a list that missed salp_food_reg.h)."""
    import glob
    return sorted(glob.glob(os.path.join(HERE, "*.h")) + glob.glob(os.path.join(HERE, "*.hip")) +
                  glob.glob(os.path.join(INCLUDE, "*.h")))


def sources() -> list:
    """Every csrc/*.hip, one compiler process each: salp_vec.hip, salp_robot.hip and the rollout kernel units
    salp_rollout_*.hip (the instantiations of salp_rollout_kernel.h, sliced so that they compile in parallel)."""
    import glob
    return sorted(glob.glob(os.path.join(HERE, "*.hip")))


OUT = os.path.join(HERE, "libsalp_hip.so")
# -ffp-contract=off: the fp64 state update must round exactly where the reference rounds
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function"]
# Per-source flags.  The rollout kernel units (and salp_vec.hip, as before the kernel moved out of it): machine LICM
# hoists every fp64 literal of the step loop (each one an s_mov pair or a v_mov pair) into registers that then live across the whole loop — ~45 VGPRs of polynomial
# coefficients and >100 SGPRs, the latter spilled to VGPR lanes and read back with v_readlane in the loop.
# Without it the one-food kernel needs 92 VGPRs / 76 SGPRs and no scratch (was 128 / 106 + 38 spilled + 20 B
# scratch), the 12-food kernel 107 VGPRs (was 160).  Measured: profiles/r02/ab_notes.md.
SRC_FLAGS = {src: ([] if src == SRC_ROBOT else ["-mllvm", "-disable-machine-licm"]) for src in sources()}


def max_jobs() -> int:
    """Compilers run at once: MAX_JOBS when set, else the CPU count; never more than 16."""
    try:
        n = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("hipcc not found")


def source_hash(defines=(), extra_flags=()) -> str:
    """sha256 over the contents of every dependency, the compiler flags and the defines: what the built library is a
    function of.  Stored next to the library (`<out>.hash`); a library whose stored hash differs is stale whatever the
    file times say (prebuilt .so files travel to the GPU box with the snapshot, where mtimes mean nothing)."""
    import hashlib
    h = hashlib.sha256()
    for d in deps():
        h.update(os.path.basename(d).encode() + b"\0")
        with open(d, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(repr((FLAGS, sorted((os.path.basename(k), v) for k, v in SRC_FLAGS.items()), list(defines), list(extra_flags))).encode())
    return h.hexdigest()


def is_current(out: str = OUT, defines=(), extra_flags=()) -> bool:
    try:
        with open(out + ".hash") as f:
            return os.path.isfile(out) and f.read().strip() == source_hash(defines, extra_flags)
    except OSError:
        return False


def stop(jobs, sig) -> None:
    """Signals the process group of every job that has not been reaped (a reaped pid is no longer ours to signal)."""
    for _, p, _ in jobs:
        if p.poll() is None:
            try:
                os.killpg(p.pid, sig)
            except ProcessLookupError:
                pass


def build(force: bool = False, verbose: bool = False, out: str = OUT, defines=(), extra_flags=()) -> str:
    """`out`/`defines`/`extra_flags` build experiment variants (profiles/ab_bench.py); the product is the default."""
    if not force and is_current(out, defines, extra_flags):
        return out
    digest = source_hash(defines, extra_flags)
    import signal
    import time
    objs, queue, running, failed = [], [], [], None
    for src in sources():             # one compile per source (different flags), max_jobs() at a time, then link
        obj = out + "." + os.path.splitext(os.path.basename(src))[0] + ".o"
        queue.append([hipcc()] + FLAGS + SRC_FLAGS[src] + list(extra_flags) + [f"-D{d}" for d in defines] + ["-c", "-o", obj, src])
        objs.append(obj)
    try:
        while running or (queue and not failed):
            while queue and not failed and len(running) < max_jobs():
                cmd = queue.pop(0)
                if verbose:
                    print(" ".join(cmd), flush=True)
                # a process group of its own: hipcc starts clang processes, which must go with it when it is stopped
                running.append((cmd, subprocess.Popen(cmd, cwd=HERE, start_new_session=True), time.monotonic()))
            time.sleep(0.05)
            done = [j for j in running if j[1].poll() is not None]
            running = [j for j in running if j not in done]       # only live compilers are ever signalled
            for cmd, p, t0 in done:
                if verbose:
                    print(f"[{time.monotonic() - t0:6.1f} s] {os.path.basename(cmd[-1])}", flush=True)
                if p.returncode != 0 and not failed:      # start no more and stop the others before raising
                    failed = subprocess.CalledProcessError(p.returncode, cmd)
                    stop(running, signal.SIGTERM)
    finally:                          # whatever ended the loop (an interrupt too), no compiler is left running
        stop(running, signal.SIGKILL)
        for _, q, _ in running:
            q.wait()
        if failed or running:         # per-object temporaries of a build that did not finish
            for o in objs:
                if os.path.exists(o):
                    os.remove(o)
    if failed:
        raise failed
    link = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True, cwd=HERE)
    for o in objs:
        os.remove(o)
    with open(out + ".hash", "w") as f:
        f.write(digest + "\n")
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--force"]
    out, defs, extra = OUT, [], []
    for a in args:
        if a.startswith("--out="):
            out = os.path.abspath(a[6:])
        elif a.startswith("-D"):
            defs.append(a[2:])
        elif a.startswith("--flag="):       # e.g. --flag=-mllvm --flag=-disable-machine-licm
            extra.append(a[7:])
    print(build(force="--force" in sys.argv, verbose=True, out=out, defines=defs, extra_flags=extra))
