#!/usr/bin/env python3
"""Registers / LDS / scratch of every salp_rollout_kernel instantiation of a built libsalp_hip.so, from the code object's
own metadata (no GPU needed): the gfx950 code objects are taken out of the library's fat binary (llvm-objcopy,
clang-offload-bundler) and their AMDGPU metadata notes read with llvm-readelf.  One line per kernel, sorted, so that two
libraries are compared with `diff`.  usage:
    python profiles/kernel_metadata.py LIB.so [--sig N] [--act N]       (filters on the SIG / ACT template arguments)
    python profiles/kernel_metadata.py LIB.so --robot                   (salp_robot_rollout_kernel<ACT, M[, SIG]> instead)
waves_per_simd = min(8, 512 / registers allocated in granules of 8, 160 KiB / LDS per workgroup of four wavefronts)."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


SNAKE = r"salp_rollout_kernelILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELi(\d+)ELb(\d)ELi(\d+)E"
ROBOT = r"salp_robot_rollout_kernelILi(\d+)ELi(\d+)E(?:Li(\d+)E)?"      # SIG: absent in libraries from before the summary signature


def kernels(lib, pattern=SNAKE):
    """The .hip_fatbin section holds one bundle per translation unit (salp_vec.hip, salp_robot.hip, every rollout kernel
    unit), each starting with MAGIC: the gfx950 code object of every one of them is read."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "copy.so")], check=True)
        with open(fat, "rb") as f:
            data = f.read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for a, b in zip(starts, starts[1:] + [len(data)]):
            with open(fat, "wb") as f:
                f.write(data[a:b])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={fat}", f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            if "amdhsa.kernels:" in notes:
                out += code_object_kernels(notes, pattern)
    return sorted(out)


def code_object_kernels(notes, pattern=SNAKE):
    md = notes[notes.index("amdhsa.kernels:"):]
    out = []
    for blk in md.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        t = re.search(pattern, name)
        if not t:
            continue
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        regs, lds = g("vgpr_count"), g("group_segment_fixed_size")
        alloc = max(8, (regs + 7) // 8 * 8)
        waves = min(8, 512 // alloc, (160 * 1024) // lds if lds else 8)
        out.append((tuple(int(x or 0) for x in t.groups()),
                    f"vgpr={regs} agpr={g('agpr_count')} sgpr={g('sgpr_count')} lds={lds} scratch={g('private_segment_fixed_size')} waves_per_simd={waves}"))
    return out


def main():
    lib, sig, act = sys.argv[1], None, None
    it = iter(sys.argv[2:])
    for a in it:
        if a == "--robot":
            for t, line in kernels(lib, ROBOT):
                print("<ACT %d, M %3d, SIG %d> " % t + line)
            return
        if a == "--sig": sig = int(next(it))
        elif a == "--act": act = int(next(it))
    for t, line in kernels(lib):
        if (sig is None or t[4] == sig) and (act is None or t[6] == act):
            print("<" + ", ".join(str(x) for x in t) + "> " + line)


if __name__ == "__main__":
    main()
