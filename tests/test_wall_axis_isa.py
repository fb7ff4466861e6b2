"""Guard for the per-axis wall screen (pt_intersect.h screen_walled, EXACTNESS.md A.21, profiles/r07/README.md): the two walls of
an axis share two of their three offsets, squares and products with d, and the headline kernel forms each once.  That is worth
20 plain instructions on each of the four secondary bounces, and nothing else may pay for it: no more transcendental or
half-rate instructions, no more registers, no more scratch.  Compiles pt_kernel.hip to gfx950 assembly on the CPU (no GPU) and
prices the hot path the way tools/isa_lines.py does.

The yardstick is the PARENT build's hot path under the same compiler (the build before this change, measured with this file's
own `profile`); like tests/test_isa_rates.py the comparison is per compiler version, and a compiler without a record skips,
printing what it measured."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "pixel_kernelILi0ELi6ELb0ELi5ELb0ELb0ELb0ELb0E"  # pixel_kernel<XORWOW, 6, false, 5>, plain: the headline build
# tools/isa_lines.py: measured issue cycles per wave64 instruction of each class, and the classes
COST = {"full": 2.2, "half": 4.0, "trans32": 8.1, "trans64": 16.2}
FULL = ("v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_fma_f32", "v_fmac_f32", "v_fmaak_f32", "v_fmamk_f32", "v_mov_b32",
        "v_xor_b32", "v_and_b32", "v_or_b32", "v_not_b32", "v_bitop3_b32", "v_lshrrev_b32", "v_ashrrev_i32", "v_add_u32", "v_sub_u32",
        "v_subrev_u32")
T32 = ("v_rcp_f32", "v_sqrt_f32", "v_rsq_f32", "v_sin_f32", "v_cos_f32", "v_exp_f32", "v_log_f32")
T64 = ("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64")
# the parent commit's headline kernel, by compiler
PARENT = {
    "7.2.26015-fc0010cf6a": {"valu": 2714, "cycles": 7572, "half": 516, "trans32": 95, "trans64": 8, "v_sqrt_f32": 38, "v_rcp_f32": 41,
                             "vgpr": 96, "scratch": 96},
}
SAVING = 80  # 4 secondary bounces x (6 + 6 + 8): per axis two subtractions and four products, on z also the two leading sums


def compiler_id():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version: (\S+)", out)
    return m.group(1) if m else "unknown"


def profile(asm):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and KERNEL in l and l.split(";")[0].rstrip().endswith(":"))
    body = []
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        body.append(l)
    loop = next(i for i, l in enumerate(body) if "This Loop Header: Depth=1" in l)
    cold = next(i for i, l in enumerate(body) if i > loop and "v_div_scale_f64" in l)
    while not body[cold].startswith(".LBB"):
        cold -= 1
    rec = {"valu": 0, "cycles": 0.0, "full": 0, "half": 0, "trans32": 0, "trans64": 0, "v_sqrt_f32": 0, "v_rcp_f32": 0}
    for l in body[loop:cold]:
        t = l.split(";")[0].strip().split()
        if not t or not t[0].startswith("v_"):
            continue
        op = t[0]
        k = "trans64" if op.startswith(T64) else "trans32" if op.startswith(T32) else "full" if op.startswith(FULL) else "half"
        rec["valu"] += 1
        rec["cycles"] += COST[k]
        rec[k] += 1
        for name in ("v_sqrt_f32", "v_rcp_f32"):
            rec[name] += op.startswith(name)
    d = next(i for i, l in enumerate(lines) if l.strip().startswith(".amdhsa_kernel ") and KERNEL in l)
    for l in lines[d:]:
        t = l.split()
        if t and t[0] == ".end_amdhsa_kernel":
            break
        if t and t[0] == ".amdhsa_next_free_vgpr":
            rec["vgpr"] = int(t[1])
        if t and t[0] == ".amdhsa_private_segment_fixed_size":
            rec["scratch"] = int(t[1])
    return rec


@pytest.fixture(scope="module")
def measured():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pt_kernel.s")
        subprocess.run(["bash", os.path.join(ROOT, "tools", "isa.sh"), out], check=True, timeout=900, capture_output=True)
        got = profile(open(out).read())
    print("headline kernel, hot path:", got)
    return got


@pytest.fixture(scope="module")
def parent(measured):
    cid = compiler_id()
    if cid not in PARENT:
        pytest.skip(f"no record of the parent build under hipcc {cid}; measured {measured}")
    return PARENT[cid]


def test_the_shared_terms_are_gone_from_the_hot_path(measured, parent):
    assert measured["valu"] <= parent["valu"] - SAVING, (measured, parent)
    # whole cycles on both sides, as tools/isa_lines.py prints them
    assert round(measured["cycles"]) <= parent["cycles"] - round(SAVING * COST["full"]), (measured, parent)


def test_nothing_slower_took_their_place(measured, parent):
    for k in ("v_sqrt_f32", "v_rcp_f32", "trans32", "trans64", "half"):
        assert measured[k] <= parent[k], (k, measured, parent)


def test_registers_and_scratch(measured, parent):
    assert measured["vgpr"] == 96, measured  # five waves per SIMD
    assert measured["scratch"] <= parent["scratch"], (measured, parent)
