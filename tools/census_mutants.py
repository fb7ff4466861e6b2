#!/usr/bin/env python3
"""Builds deliberately wrong lab libraries of the pixel kernels, to show that tests/test_kernel_census_gpu.py can fail
(profiles/kernel_census/README.md).  Each mutant is a textual change of a COPY of csrc/pt_kernel.hip -- the committed source and
the product build know nothing of it -- linked with the unchanged lab objects into
cuda-pathtrace_amd/alt/census_mutant<n>/libptcore_lab.so (alt/ is not in git).  A mutant changes a host-side choice or a value
only: no address and no bound of a load or store.

  1  selector: variant_kernel hands out the GENERIC build where the 8-bounce reference configuration was asked for (plain, resume
     and adaptive flavours; a batch has no generic build).  The bits stay the oracle's, so no parity test can see it; the census
     cases of the REFB = 8 builds must fail on the build that ran.
  2  value: the non-lean resume build of row 10 (pixel_kernel<RNG, 10, false, 0, false, false, true, false>, confined by
     `if constexpr`) stores its record's first colour sum one ulp up.  Its census case must fail on parity from the second pass
     on; tests/test_progressive_gpu.py and tests/test_adaptive_gpu.py, which never launch that build, pass.

Usage: tools/census_mutants.py [1 2]   (cross-compiles for gfx950; no GPU needed).  To run the tests against a mutant, put its
library in the place of cuda-pathtrace_amd/libptcore_lab.so in a scratch copy of the tree."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtrace_amd", "csrc")
ALT = os.path.join(ROOT, "cuda-pathtrace_amd", "alt")

MUTANTS = {
    1: ("      if (ref == 8 && !lean) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 8>();\n",
        "      if (ref == 8 && !lean) {\n"
        "        if constexpr (!FRAMES) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 0>();\n"
        "        else return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 8>();\n"
        "      }\n"),
    2: ("      auto st = [&](int w, uint32_t v) { rec[(size_t)w * a.tile_pixels + tp] = v; };\n",
        "      auto st = [&](int w, uint32_t v) { rec[(size_t)w * a.tile_pixels + tp] = v; };\n"
        "      if constexpr (VAR == 10 && !LEAN && !ADAPTIVE) L.color.x = __uint_as_float(__float_as_uint(L.color.x) + 1u);\n"),
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
    common = os.path.join(ALT, "census_mutant_common")
    os.makedirs(common, exist_ok=True)
    source = open(os.path.join(CSRC, "pt_kernel.hip")).read()
    for n in which:
        if source.count(MUTANTS[n][0]) != 1:
            raise SystemExit(f"mutant {n}: the line to change occurs {source.count(MUTANTS[n][0])} times in pt_kernel.hip, not once")

    def compile_one(src, obj, extra=()):
        subprocess.check_call([hipcc] + flags + list(extra) + ["-c", src, "-o", obj])
        return obj

    def mutant(n):
        out = os.path.join(ALT, f"census_mutant{n}")
        os.makedirs(out, exist_ok=True)
        # two levels below the repository root, like csrc/, so that the source's relative includes still resolve
        src = os.path.join(ALT, f"pt_kernel_mutant{n}.hip")
        with open(src, "w") as f:
            f.write(source.replace(*MUTANTS[n]))
        return n, out, compile_one(src, os.path.join(out, "pt_kernel.o"), [f'-DPT_BUILD_FINGERPRINT="census-mutant{n}"'])

    with ThreadPoolExecutor(max_workers=4) as pool:
        kernels = [pool.submit(mutant, n) for n in which]  # (the long compilations first)
        jobs = [pool.submit(compile_one, os.path.join(CSRC, s), os.path.join(common, s + ".o"), ['-DPT_BUILD_FINGERPRINT="census-mutant"'])
                for s in srcs if s != "pt_kernel.hip"]
        objs = [j.result() for j in jobs]
        for k in kernels:
            n, out, obj = k.result()
            lib = os.path.join(out, "libptcore_lab.so")
            subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + [obj, "-ldl", "-lpthread"])
            print(f"mutant {n}: {lib}")


if __name__ == "__main__":
    main()
