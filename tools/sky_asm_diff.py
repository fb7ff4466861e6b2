#!/usr/bin/env python3
"""Compare the function bodies of pixel_kernel_materials<RNG, LIGHTS> in two gfx950 assembly files of csrc/pt_materials.hip
(the `-save-temps` output of two builds, e.g. csrc/build/prod/pt_materials-hip-amdgcn-amd-amdhsa-gfx950.s of the parent commit
and of this one): profiles/sky/README.md.

A body is everything between the kernel's label and its .Lfunc_end.  Removed before comparing: comments, the kernel's mangled name, the function ordinal
in block labels (.LBB<ordinal>_<block>) and blank lines.  Prints one line per instantiation; exit status 1 if any differs.

usage: sky_asm_diff.py PARENT.s THIS.s"""
import difflib
import re
import sys

# the parent's <RNG, LIGHTS> and this commit's <RNG, LIGHTS, false> (an empty argument pack: "ELb0EJEEE")
KERNEL = re.compile(r"^_ZN2pt9materials22pixel_kernel_materialsILi(\d)ELb(\d)E(?:Lb0EJE)?EEv\S*:")


def bodies(path):
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = KERNEL.match(line)
            if m and cur is None:
                cur = out.setdefault(("XORWOW" if m.group(1) == "0" else "Philox", "LIGHTS" if m.group(2) == "1" else "plain"), [])
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            line = re.sub(r"_ZN2pt9materials22pixel_kernel_materialsI\w+", "KERNEL", line.split(";")[0])
            line = re.sub(r"\.LBB\d+_", ".LBB_", line).rstrip()
            if line:
                cur.append(line)
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    differs = False
    for key in sorted(a):
        if key not in b:
            print(key, "missing from", sys.argv[2])
            differs = True
            continue
        same = a[key] == b[key]
        differs |= not same
        print("%-7s %-6s %5d / %5d lines: %s" % (key[0], key[1], len(a[key]), len(b[key]), "identical" if same else "DIFFERENT"))
        if not same:
            for i, l in enumerate(difflib.unified_diff(a[key], b[key], lineterm="", n=0)):
                if i > 30:
                    break
                print("   ", l)
    return 1 if differs or len(a) != 4 else 0


if __name__ == "__main__":
    sys.exit(main())
