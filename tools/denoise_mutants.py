#!/usr/bin/env python3
"""Builds deliberately wrong lab libraries of the denoiser, to show that tests/test_denoiser_exact_gpu.py can fail
(profiles/denoise_exact/README.md).  Each mutant is a one-line textual change of a COPY of csrc/pt_denoise.hip -- the
committed source and the product build know nothing of it -- linked with the unchanged lab objects into
cuda-pathtrace_amd/alt/denoise_mutant<n>/libptcore_lab.so (alt/ is not in git).  A mutant changes values only: no address, no
bound of a load or store; mutant 2 launches FEWER K slices of the same size, over the same buffers.

  1  upsample(): the row weight is divided by out_w - 1 instead of out_h - 1 (the row index is unchanged): invisible at any
     square size.
  2  choose_tiles(): splits = nchunks / chunks_per_split, floor instead of ceil: a short last K slice is dropped; invisible
     wherever the slices are even.
  3  conv_kernel's window origin: iy0 one row higher where a stride-2 layer reads a map of odd height that is not square (the
     loads stay bounds-checked): invisible at any square size.

Usage: tools/denoise_mutants.py [1 2 3]   (cross-compiles for gfx950; no GPU needed).  To run the tests against a mutant, put
its library in the place of cuda-pathtrace_amd/libptcore_lab.so in a scratch copy of the tree."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtrace_amd", "csrc")
ALT = os.path.join(ROOT, "cuda-pathtrace_amd", "alt")

MUTANTS = {
    1: ("h1l = (float)(q - h1 * (a.out_h - 1)) / (float)(a.out_h - 1);",
        "h1l = (float)(q - h1 * (a.out_h - 1)) / (float)(a.out_w - 1);"),
    2: ("c.splits = (c.nchunks + c.chunks_per_split - 1) / c.chunks_per_split;",
        "c.splits = c.nchunks / c.chunks_per_split;"),
    3: ("iy0[i] = oy * a.stride - pad;",
        "iy0[i] = oy * a.stride - pad - ((a.stride == 2 && (a.in_h & 1) && a.in_h != a.in_w) ? 1 : 0);"),
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
    common = os.path.join(ALT, "denoise_mutant_common")
    os.makedirs(common, exist_ok=True)

    def compile_one(src, obj, extra=()):
        subprocess.check_call([hipcc] + flags + list(extra) + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:
        jobs = [pool.submit(compile_one, os.path.join(CSRC, s), os.path.join(common, s + ".o"), ['-DPT_BUILD_FINGERPRINT="denoise-mutant"'])
                for s in srcs if s != "pt_denoise.hip"]
        objs = [j.result() for j in jobs]
    source = open(os.path.join(CSRC, "pt_denoise.hip")).read()
    for n in which:
        old, new = MUTANTS[n]
        if source.count(old) != 1:
            raise SystemExit(f"mutant {n}: the line to change occurs {source.count(old)} times in pt_denoise.hip, not once")
        out = os.path.join(ALT, f"denoise_mutant{n}")
        os.makedirs(out, exist_ok=True)
        # two levels below the repository root, like csrc/, so that the source's relative includes still resolve
        src = os.path.join(ALT, f"pt_denoise_mutant{n}.hip")
        with open(src, "w") as f:
            f.write(source.replace(old, new))
        obj = compile_one(src, os.path.join(out, "pt_denoise.o"), [f'-DPT_BUILD_FINGERPRINT="denoise-mutant{n}"'])
        lib = os.path.join(out, "libptcore_lab.so")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + [obj, "-ldl", "-lpthread"])
        print(f"mutant {n}: {lib}")


if __name__ == "__main__":
    main()
