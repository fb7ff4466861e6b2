#!/usr/bin/env python3
"""Builds deliberately wrong lab libraries of the adaptive stage, to show that tests/test_adaptive_exact_gpu.py can fail
(profiles/adaptive_exact/README.md).  Each mutant is a one-line textual change of a COPY of csrc/pt_adaptive.hip -- the
committed source and the product build know nothing of it -- linked with the unchanged lab objects into
cuda-pathtrace_amd/alt/adaptive_mutant<n>/libptcore_lab.so (alt/ is not in git).  A mutant changes values or decisions only: no
index grows and no bound of a load or store moves.  The two scan mutants LOSE an offset, so list slots only get smaller.

  1  scan: the previous waves' totals are summed with w + 1 < wave, so every wave but the first loses the total of the wave
     before it: invisible up to 64 blocks of 256 pixels (16384 pixels).
  2  scan: the write-back loop does not advance the running prefix, so a lane's second and later blocks get the prefix of its
     first: invisible up to 1024 blocks (262144 pixels), where every lane holds one block.
  3  rule: <= becomes <: a variance exactly at the threshold no longer converges.
  4  rule: the floor is ignored (m = lum).
  5  dilation: the window looks for an ACTIVE pixel (mask bit 0) instead of an unconverged one (bit 1).

With mutants 1 and 2 a session's pass would read list slots nobody wrote, so run them only against tests that look at the list
and never render from it (tests/test_adaptive_exact_gpu.py), or against sessions of at most 64 (1024) blocks.

Usage: tools/adaptive_mutants.py [1 2 3 4 5]   (cross-compiles for gfx950; no GPU needed).  To run the tests against a mutant,
put its library in the place of cuda-pathtrace_amd/libptcore_lab.so in a scratch copy of the tree."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtrace_amd", "csrc")
ALT = os.path.join(ROOT, "cuda-pathtrace_amd", "alt")

MUTANTS = {
    1: ("if (w < wave) off += s_waves[w];", "if (w + 1 < wave) off += s_waves[w];"),
    2: ("    run += v;\n", "    run += 0u * v;\n"),
    3: ("conv = (double)px[10] <= ((rule.tolerance", "conv = (double)px[10] < ((rule.tolerance"),
    4: ("const double m = (double)lum > rule.floor ? (double)lum : rule.floor;", "const double m = (double)lum;"),
    5: ("if (mask[(size_t)y * width + x] & 2u) {", "if (mask[(size_t)y * width + x] & 1u) {"),
}


def make_var(text, name):
    m = re.search(r"^%s\s*=\s*(.*)$" % re.escape(name), text, re.M)
    if not m:
        raise SystemExit(f"csrc/Makefile: no {name}")
    return m.group(1).strip()


def main():
    which = [int(a) for a in sys.argv[1:]] or sorted(MUTANTS)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950"] + make_var(mk, "CXXFLAGS").split() + ["-DPT_BUILD_EXPERIMENTS=1", "-I" + CSRC]
    srcs = make_var(mk, "SRCS").split() + ["pt_debug.hip"]
    common = os.path.join(ALT, "adaptive_mutant_common")
    os.makedirs(common, exist_ok=True)

    def compile_one(src, obj, extra=()):
        subprocess.check_call([hipcc] + flags + list(extra) + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:
        jobs = [pool.submit(compile_one, os.path.join(CSRC, s), os.path.join(common, s + ".o"), ['-DPT_BUILD_FINGERPRINT="adaptive-mutant"'])
                for s in srcs if s != "pt_adaptive.hip"]
        objs = [j.result() for j in jobs]
    source = open(os.path.join(CSRC, "pt_adaptive.hip")).read()
    for n in which:
        old, new = MUTANTS[n]
        if source.count(old) != 1:
            raise SystemExit(f"mutant {n}: the line to change occurs {source.count(old)} times in pt_adaptive.hip, not once")
        out = os.path.join(ALT, f"adaptive_mutant{n}")
        os.makedirs(out, exist_ok=True)
        # two levels below the repository root, like csrc/, so that the source's relative includes still resolve
        src = os.path.join(ALT, f"pt_adaptive_mutant{n}.hip")
        with open(src, "w") as f:
            f.write(source.replace(old, new))
        obj = compile_one(src, os.path.join(out, "pt_adaptive.o"), [f'-DPT_BUILD_FINGERPRINT="adaptive-mutant{n}"'])
        lib = os.path.join(out, "libptcore_lab.so")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + [obj, "-ldl", "-lpthread"])
        print(f"mutant {n}: {lib}")


if __name__ == "__main__":
    main()
