#!/usr/bin/env python3
"""Are the kernels of two sets of gfx950 assembly dumps (profiles/isa_dump.sh) the same machine code?  Every kernel's body
and its .amdhsa_kernel descriptor are compared by name after stripping comments, renaming local labels (their numbers
count the functions of the dump, so they differ between a whole-file dump and the dumps of the units) and collapsing
whitespace.  usage:
    python profiles/isa_kernel_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]
Prints the kernel counts and every name that is missing, doubled or different; exit status 1 if there is one."""
import re, sys


def norm(line):
    line = line.split(";", 1)[0]
    line = re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+", r".L\1", line)
    return " ".join(line.split())


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
    (old, d_old), (new, d_new) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = [f"doubled: {k}" for k in d_old + d_new]
    bad += [f"only in old: {k}" for k in sorted(set(old) - set(new))] + [f"only in new: {k}" for k in sorted(set(new) - set(old))]
    bad += [f"differs: {k}" for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    rollout = sum("salp_rollout_kernel" in k for k in new)
    print(f"old: {len(old)} kernels, new: {len(new)} kernels ({rollout} rollout, {len(new) - rollout} service), "
          f"{sum(len(v) for v in new.values())} lines compared, {len(bad)} problems")
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
