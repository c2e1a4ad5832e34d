#!/usr/bin/env python3
"""Are the kernels of two sets of gfx950 assembly dumps (profiles/isa_dump.sh) the same machine code?  Every kernel's body
and its .amdhsa_kernel descriptor are compared by name after stripping comments, renaming local labels (their numbers
count the functions of the dump, so they differ between a whole-file dump and the dumps of the units) and collapsing
whitespace.  usage:
    python profiles/isa_kernel_diff.py [--modulo-registers] OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]
Prints the kernel counts and every name that is missing, doubled or different; exit status 1 if there is one.

--modulo-registers: two verdicts per kernel.  (a) the bodies are identical, as without the option;  (b) they are identical
as MULTISETS of instructions after every register operand is replaced by its class and width (v[4:5] -> v<2>, s17 -> s<1>,
a[0:3] -> a<4>) and every block label by `.LBB` (block numbers follow the order of the blocks): the same instructions,
possibly in another order and in other registers, which is what regrouping a kernel's locals without changing what it
computes does to the register allocator and the scheduler.  Opcodes, immediates, modifiers and the special registers
(vcc, exec, m0) stay as they are, so a value that moved between vcc and an SGPR pair counts as different.  The .amdhsa_kernel
descriptor (register counts, LDS, scratch, ...) is compared exactly in both.  The names that fail (a) alone are listed as
`reordered`, the names that fail (b) or the descriptor as `differs`; exit status 1 only if something `differs`."""
import re, sys
from collections import Counter


def norm(line):
    line = line.split(";", 1)[0]
    line = re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+", r".L\1", line)
    return " ".join(line.split())


REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def erase_registers(line):
    """Every register operand by class and width; labels, opcodes, immediates and modifiers stay."""
    line = re.sub(r"\.L(BB|JTI)_?\d+(_\d+)?", r".L\1", line)       # block numbers follow the order of the blocks
    return REG.sub(lambda m: f"{m.group(1)}<{1 if m.group(2) is not None else int(m.group(4)) - int(m.group(3)) + 1}>", line)


def split(lines):
    """(body, descriptor) of one kernel's normalised lines."""
    d = next((i for i, ln in enumerate(lines) if ln.startswith(".amdhsa_kernel ")), len(lines))
    return lines[:d], lines[d:]


def same_modulo_registers(old, new):
    (bo, do), (bn, dn) = split(old), split(new)
    return do == dn and Counter(map(erase_registers, bo)) == Counter(map(erase_registers, bn))


def kernels(paths):
    out, doubled = {}, []
    for path in paths.split(","):
        lines = open(path).read().split("\n")
        names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
        cur = None
        for ln in lines:
            m = re.match(r"^(\S+):", ln)
            d = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
            if cur is None and ((m and m.group(1) in names) or d):
                cur = (m or d).group(1)
                if m and cur in out:
                    doubled.append(cur)
                out.setdefault(cur, [])
            if cur is not None:
                n = norm(ln)
                if n:
                    out[cur].append(n)
                if re.match(r"^\.Lfunc_end\d+:", ln) or re.match(r"^\s*\.end_amdhsa_kernel", ln):
                    cur = None
    return out, doubled


def main():
    args = [a for a in sys.argv[1:] if a != "--modulo-registers"]
    modulo = len(args) != len(sys.argv) - 1
    (old, d_old), (new, d_new) = kernels(args[0]), kernels(args[1])
    bad = [f"doubled: {k}" for k in d_old + d_new]
    bad += [f"only in old: {k}" for k in sorted(set(old) - set(new))] + [f"only in new: {k}" for k in sorted(set(new) - set(old))]
    changed = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    reordered = [k for k in changed if modulo and same_modulo_registers(old[k], new[k])]
    bad += [f"differs: {k}" for k in changed if k not in reordered]
    rollout = sum("salp_rollout_kernel" in k for k in new)
    print(f"old: {len(old)} kernels, new: {len(new)} kernels ({rollout} rollout, {len(new) - rollout} service), "
          f"{sum(len(v) for v in new.values())} lines compared, {len(bad)} problems")
    if modulo:
        both = len(set(old) & set(new))
        print(f"identical (a): {both - len(changed)} of {both}; identical modulo registers and order (b): "
              f"{both - len(changed) + len(reordered)} of {both}")
        print("\n".join(f"reordered: {k}" for k in reordered))
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
