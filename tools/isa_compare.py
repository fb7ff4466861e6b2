#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds, kernel by kernel: is the device code the same?

    tools/isa_compare.py OLD_DIR NEW_DIR      (the build/prod or build/lab directories csrc/Makefile leaves)

For every *-gfx950.s of both directories: the set of kernel symbols, each function's instruction stream (comments, .loc / .file
lines and blank lines dropped, local labels renumbered in order of appearance) and each .amdhsa_kernel descriptor block.
Prints one line per object and every difference; exit status 1 if anything differs.  Text only: needs no GPU.
"""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse(path):
    """-> ({function: [normalised lines]}, {kernel: [descriptor lines]})"""
    funcs, descs = {}, {}
    cur = body = labels = desc = None
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        text = line.strip()
        if desc is not None:
            if text == ".end_amdhsa_kernel":
                desc = None
            elif text:
                desc.append(text)
            continue
        if text.startswith(".amdhsa_kernel "):
            desc = descs.setdefault(text.split()[1], [])
            continue
        if cur is None:
            if re.match(r"^[A-Za-z_][\w$.]*:$", line) and not line.startswith(".L"):
                cur, body, labels = line[:-1], [], {}
            continue
        if text.startswith(".Lfunc_end"):
            funcs[cur] = body
            cur = None
            continue
        if not text or text.startswith((".loc", ".file", ".cfi_")):
            continue
        body.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), text))
    return funcs, descs


def main(old_dir, new_dir):
    bad = 0
    names = lambda d: {os.path.basename(p) for p in glob.glob(os.path.join(d, "*-gfx950.s"))}
    old_names, new_names = names(old_dir), names(new_dir)
    for n in sorted(old_names ^ new_names):
        print("object only on one side:", n)
        bad += 1
    for n in sorted(old_names & new_names):
        (fo, do), (fn, dn) = parse(os.path.join(old_dir, n)), parse(os.path.join(new_dir, n))
        diffs = ["kernel only in old: " + k for k in sorted(set(do) - set(dn))] + ["kernel only in new: " + k for k in sorted(set(dn) - set(do))]
        diffs += ["function only in old: " + k for k in sorted(set(fo) - set(fn))] + ["function only in new: " + k for k in sorted(set(fn) - set(fo))]
        for k in sorted(set(fo) & set(fn)):
            if fo[k] != fn[k]:
                diffs.append("instructions differ: %s (%d -> %d lines)" % (k, len(fo[k]), len(fn[k])))
        for k in sorted(set(do) & set(dn)):
            if do[k] != dn[k]:
                diffs.append("descriptor differs: " + k)
        missing = [k for k in dn if k not in fn]
        diffs += ["kernel without a body: " + k for k in missing]
        instr = sum(len(fn[k]) for k in dn if k in fn)
        print("%-24s %3d kernels, %8d lines in them: %s" % (n.split("-hip-")[0], len(dn), instr, "identical" if not diffs else "%d DIFFERENCES" % len(diffs)))
        for d in diffs:
            print("   ", d)
        bad += len(diffs)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
