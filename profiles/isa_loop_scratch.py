#!/usr/bin/env python3
"""Which loops of a kernel touch scratch memory?  Reads a gfx950 assembly dump (profiles/isa_dump.sh, or hipcc -S
--cuda-device-only) and lists, for every kernel whose name contains PATTERN, its loops — found by their backward branches
in layout order — with their size, their fp64 instruction count and the number of scratch loads / stores inside.
    python profiles/isa_loop_scratch.py DUMP.s [PATTERN]
Used for profiles/robot_rollout_notes.md: the loop of salp_robot_rollout_kernel that holds the Euler step (the one with
448 fp64 instructions) must show 0 scratch accesses."""
import re
import sys


def kernels(lines):
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    for i, ln in enumerate(lines):
        m = re.match(r"^(\S+):", ln)
        if m and m.group(1) in names:
            end = next(k for k in range(i, len(lines)) if re.match(r"^\.Lfunc_end", lines[k]))
            yield m.group(1), lines[i + 1:end]


def loops(body):
    blocks = [["entry", []]]
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append([m.group(1), []])
            continue
        t = ln.strip()
        if t and not t.startswith(";") and not t.startswith("."):
            blocks[-1][1].append(t)
    index = {b[0]: k for k, b in enumerate(blocks)}
    found = set()
    for k, (_, ins) in enumerate(blocks):
        for t in ins:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
            if m and index[m.group(1)] <= k:
                found.add((index[m.group(1)], k))
    for a, b in sorted(found):
        ins = [t for _, block in blocks[a:b + 1] for t in block]
        yield (blocks[a][0], blocks[b][0], b - a + 1, len(ins), sum(bool(re.match(r"v_\w+_f64", t)) for t in ins),
               sum(t.startswith("scratch_") for t in ins))


def main():
    pattern = sys.argv[2] if len(sys.argv) > 2 else ""
    lines = open(sys.argv[1]).read().split("\n")
    for name, body in kernels(lines):
        if pattern in name:
            print(name)
            for first, last, n_blocks, n_ins, f64, scratch in loops(body):
                print(f"  loop {first} .. {last}: {n_blocks} blocks, {n_ins} instructions, {f64} fp64, {scratch} scratch accesses")


if __name__ == "__main__":
    main()
