#!/usr/bin/env python3
"""Development aid: per-kernel diff of two device listings of one .hip file (two commits, two spellings of one kernel).
Comments, directives and the per-build __hip_cuid_* symbol are dropped and temporary labels are numbered by first use;
each kernel is then "identical", "multiplicands exchanged only" (the lines that differ are FMAs / multiplies with src0 and
src1 swapped: the same bits) or "differs", with both builds' registers, LDS and private segment from the metadata.
usage: hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S -o new.s ga3c_amd/csrc/ga3c_mlp.hip   (and old.s)
       tools/asm_diff.py old.s new.s [-v]        (-v: the differing lines of every kernel that differs)"""
import re
import subprocess
import sys

FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
COMMUTE = re.compile(r"v_(pk_)?(fma|fmac|mul|add)_f32")


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    lines = text.split("\n")
    body, meta = {}, {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        labels, out = {}, []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if not l or "__hip_cuid_" in l or (l.startswith(".") and not l.startswith(".LBB")):
                continue
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), l)
            out.append(re.sub(r"\s+", " ", l))
        body[name] = out
    for block in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        if ".name:" not in block:         # amdhsa.version's list, after the kernels
            continue
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        meta[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f in FIELDS)
    return body, meta


def exchanged(a, b):
    pa, pb = a.replace(",", " ").split(), b.replace(",", " ").split()
    if len(pa) != len(pb) or len(pa) < 4 or pa[0] != pb[0] or not COMMUTE.fullmatch(pa[0].replace("_e32", "").replace("_e64", "")):
        return False
    return pa[1] == pb[1] and pa[2] == pb[3] and pa[3] == pb[2] and sorted(pa[4:]) == sorted(pb[4:])


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "")


def main():
    verbose = "-v" in sys.argv
    old_path, new_path = [a for a in sys.argv[1:] if a != "-v"]
    (ob, om), (nb, nm) = kernels(old_path), kernels(new_path)
    for name in ob:
        if name not in nb:
            print("%-60s missing from %s" % (demangle(name), new_path))
            continue
        a, b = ob[name], nb[name]
        pairs = [(x, y) for x, y in zip(a, b) if x != y]
        if len(a) == len(b) and not pairs:
            verdict = "identical"
        elif len(a) == len(b) and all(exchanged(x, y) for x, y in pairs):
            verdict = "multiplicands exchanged only (%d of %d lines)" % (len(pairs), len(a))
        else:
            verdict = "differs: %d -> %d lines; " % (len(a), len(b)) + "; ".join(
                "%s %d -> %d" % (f, o, n) for f, o, n in zip(("vgpr", "sgpr", "lds", "private"), om[name], nm[name]))
        print("%-60s %s" % (demangle(name), verdict))
        if verbose and verdict.startswith("differs"):
            import difflib
            print("\n".join(difflib.unified_diff(a, b, "old", "new", n=1, lineterm="")))
    for name in nb:
        if name not in ob:
            print("%-60s new in %s" % (demangle(name), new_path))


if __name__ == "__main__":
    main()
