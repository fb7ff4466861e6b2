#!/usr/bin/env python3
"""Builds deliberately wrong product libraries of the tone-mapping, comparison and training-patch stages, to show that
tests/test_stage_sums_gpu.py can fail where the stages' own files cannot (profiles/stage_sums/README.md).  Each mutant is a
one-line textual change of a COPY of one of csrc/pt_tonemap.hip, pt_compare.hip, pt_patches.hip -- the committed sources and the
product build know nothing of it -- linked with the unchanged objects into cuda-pathtrace_amd/alt/stage_sum_mutant<n>/libptcore.so
(alt/ is not in git).  Every mutant only LOSES values: a loop stops early or a lane takes the identity instead of its load, so no
index grows and no bound of a load or store moves.

  1  tonemap adapt_kernel: the strided loop over a frame's block partials makes its first trip only (invisible up to 256 blocks,
     65536 pixels).
  2  compare sum_kernel: the strided loop over a frame's tile partials makes its first trip only (invisible up to 256 tiles).
  3  patches sum_kernel: the strided loop over a patch's chunk partials makes its first trip only (invisible up to P = 512).
  4  patches max_kernel: the grid-stride loop makes its first trip only (invisible up to 65536 pixels).
  5  patches gather_kernel: the fold of the partial maxima ignores lanes 192-255, the fourth wave (invisible up to 192 partials,
     49152 pixels); the change is in the gather's load, not in fold4, which max_kernel shares.
  6  pt_compare_result: the signed SSIM sum is read as unsigned when the double is formed (invisible while the sum is >= 0).

Usage: tools/stage_sum_mutants.py [1 2 3 4 5 6]   (cross-compiles for gfx950; no GPU needed).  To run tests against a mutant:
PT_LIB_OVERRIDE=cuda-pathtrace_amd/alt/stage_sum_mutant<n>/libptcore.so python -m pytest -m gpu tests/test_stage_sums_gpu.py"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtrace_amd", "csrc")
ALT = os.path.join(ROOT, "cuda-pathtrace_amd", "alt")

MUTANTS = {
    1: ("pt_tonemap.hip", "for (uint32_t b = threadIdx.x; b < blocks; b += BLOCK) {",
        "for (uint32_t b = threadIdx.x; b < blocks && b < BLOCK; b += BLOCK) {"),
    2: ("pt_compare.hip", "for (uint32_t b = threadIdx.x; b < tiles; b += BLOCK) {",
        "for (uint32_t b = threadIdx.x; b < tiles && b < BLOCK; b += BLOCK) {"),
    3: ("pt_patches.hip", "for (uint32_t b = threadIdx.x; b < chunks; b += BLOCK) {",
        "for (uint32_t b = threadIdx.x; b < chunks && b < BLOCK; b += BLOCK) {"),
    4: ("pt_patches.hip", "p < pixels; p += gridDim.x * (uint32_t)BLOCK)",
        "p < pixels && p < gridDim.x * (uint32_t)BLOCK; p += gridDim.x * (uint32_t)BLOCK)"),
    5: ("pt_patches.hip", "mx[k] = (int)threadIdx.x < a.nparts ? a.part",
        "mx[k] = (int)threadIdx.x < a.nparts && threadIdx.x < 192 ? a.part"),
    6: ("pt_compare.hip", "out->ssim = (double)r.qs / 4294967296.0 / px;", "out->ssim = (double)(uint64_t)r.qs / 4294967296.0 / px;"),
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
    flags = ["--offload-arch=gfx950"] + make_var(mk, "CXXFLAGS").split() + ["-I" + CSRC]
    srcs = make_var(mk, "SRCS").split()
    common = os.path.join(ALT, "stage_sum_mutant_common")
    os.makedirs(common, exist_ok=True)

    def compile_one(src, obj, fingerprint):
        subprocess.check_call([hipcc] + flags + [f'-DPT_BUILD_FINGERPRINT="{fingerprint}"', "-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:
        jobs = {s: pool.submit(compile_one, os.path.join(CSRC, s), os.path.join(common, s + ".o"), "stage-sum-mutant") for s in srcs}
        objs = {s: j.result() for s, j in jobs.items()}
    for n in which:
        name, old, new = MUTANTS[n]
        source = open(os.path.join(CSRC, name)).read()
        if source.count(old) != 1:
            raise SystemExit(f"mutant {n}: the line to change occurs {source.count(old)} times in {name}, not once")
        out = os.path.join(ALT, f"stage_sum_mutant{n}")
        os.makedirs(out, exist_ok=True)
        # two levels below the repository root, like csrc/, so that the source's relative includes still resolve
        src = os.path.join(ALT, f"stage_sum_mutant{n}_{name}")
        with open(src, "w") as f:
            f.write(source.replace(old, new))
        obj = compile_one(src, os.path.join(out, name + ".o"), f"stage-sum-mutant{n}")
        lib = os.path.join(out, "libptcore.so")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-o", lib] + [obj if s == name else objs[s] for s in srcs]
                              + ["-ldl", "-lpthread"])
        print(f"mutant {n}: {lib}")


if __name__ == "__main__":
    main()
