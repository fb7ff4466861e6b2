#!/usr/bin/env python3
"""Builds deliberately wrong lab libraries of the denoiser, to show that tests/test_denoiser_exact_gpu.py can fail
(profiles/denoise_exact/README.md).  Each mutant is a one-line textual change of a COPY of csrc/pt_denoise.hip -- the
committed source and the product build know nothing of it -- linked with the unchanged lab objects into
cuda-pathtrace_amd/alt/denoise_mutant<n>/libptcore_lab.so (alt/ is not in git).  Mutants 1-3 change values only: no address, no
bound of a load or store; mutant 2 launches FEWER K slices of the same size, over the same buffers.

  1  upsample(): the row weight is divided by out_w - 1 instead of out_h - 1 (the row index is unchanged): invisible at any
     square size.
  2  choose_tiles(): splits = nchunks / chunks_per_split, floor instead of ceil: a short last K slice is dropped; invisible
     wherever the slices are even.
  3  conv_kernel's window origin: iy0 one row higher where a stride-2 layer reads a map of odd height that is not square (the
     loads stay bounds-checked): invisible at any square size.

Mutants 4-8 show that tests/test_denoiser_groups_gpu.py can fail where a group of frames has code of its own
(profiles/denoise_groups/README.md).  Each only misplaces a read inside the workspace, or re-slices K inside the partial sums the
workspace was sized for; none leaves an allocation:

  4  half main loop: the window of every row block is read from the frame of row block 0 (iyb[0]): wrong only where a TM = 2
     tile (256x32, 128x128) holds rows of two frames.
  5  the same in the float32 main loop.
  6  set-up: the frame of every row is the frame of the wave's first row (frame_of once from m0); the loads stay bounds-checked
     inside that frame.
  7  pre_apply_kernel divides every frame of a group by the maxima of frame 0.
  8  plan_for(): the K slicing is chosen again for the group's M (fewer, longer slices; never more than the single-frame
     slicing that pt_denoiser_reserve_frames sized the partial sums for, which is why the change is made here and not in
     batch_plan() itself).  Integer sums are exact in any order: only real weights see it.

Usage: tools/denoise_mutants.py [1 2 ...]   (cross-compiles for gfx950; no GPU needed).  To run the tests against a mutant, put
its library in the place of cuda-pathtrace_amd/libptcore_lab.so in a scratch copy of the tree; tests that go through the
product library see it too when PT_LIB_OVERRIDE names the same file."""
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
    4: ("v_ = *reinterpret_cast<const half8*>(a.in + ((size_t)(iyb[i] + iy)",
        "v_ = *reinterpret_cast<const half8*>(a.in + ((size_t)(iyb[0] + iy)"),
    5: ("reinterpret_cast<const float4*>(a.in + ((size_t)(iyb[i] + iy)",
        "reinterpret_cast<const float4*>(a.in + ((size_t)(iyb[0] + iy)"),
    6: ("const int f = frame_of(a, mm), pix = mm - f * a.out_hw;",
        "const int f = frame_of(a, m0 < a.M ? m0 : 0), pix = mm - f * a.out_hw;"),
    7: ("const float* fp = part + (size_t)blockIdx.y * nparts * 5;",
        "const float* fp = part + (size_t)0 * nparts * 5;"),
    8: ("if (it == d->plans.end()) it = d->plans.emplace(n, batch_plan(d->convs, n, kPlan[d->precision])).first;",
        "if (it == d->plans.end()) { std::vector<Conv> pl = batch_plan(d->convs, n, kPlan[d->precision]); "
        "for (Conv& c : pl) { const int cfg_ = c.cfg, npad_ = c.npad; choose_tiles(c, kPlan[d->precision]); c.cfg = cfg_, c.npad = npad_; } "
        "it = d->plans.emplace(n, pl).first; }"),
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

    def build(n):
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
        return f"mutant {n}: {lib}"

    with ThreadPoolExecutor(max_workers=4) as pool:
        for line in pool.map(build, which):
            print(line)


if __name__ == "__main__":
    main()
