#!/usr/bin/env python3
"""Self-test of tests/test_primary_exclusion_gpu.py: four deliberately UNSOUND lab libraries -- -DPT_FOOTPRINT_MUTANT=1 / 2
(csrc/pt_footprint.h: footprint radius x 0.3; margin 0.93) and -DPT_PRIMLIST_MUTANT=1 / 2 (csrc/pt_primlist.h: radius x 0.3; a
sphere counts as missed inside 0.8 r) -- built with tools/build_alt.sh into cuda-pathtrace_amd/alt/primary_mutant_<f|p><n>/, and the
mask or list equality of the test run once against each.  Every one must MISMATCH the sound models (and match the model with the
mutant's constant, which shows that the constant is all that differs).  Output: profiles/primary_exclusion/.
Usage: primary_exclusion_mutants.py build       (needs hipcc, no device)
       primary_exclusion_mutants.py run         (needs the device; one fresh process per library)"""
import json, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANTS = [("f1", "PT_FOOTPRINT_MUTANT", 1, {"radius_factor": 0.3}), ("f2", "PT_FOOTPRINT_MUTANT", 2, {"margin": 0.93}),
           ("p1", "PT_PRIMLIST_MUTANT", 1, {"radius_factor": 0.3}), ("p2", "PT_PRIMLIST_MUTANT", 2, {"miss_scale": 0.64})]
lib_of = lambda tag: os.path.join(root, "cuda-pathtrace_amd", "alt", f"primary_mutant_{tag}", "libptcore_lab.so")


def build():
    mk = open(os.path.join(root, "cuda-pathtrace_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1) + " pt_debug.hip"  # the Makefile's LAB_SRCS
    procs = [subprocess.Popen([os.path.join(root, "tools", "build_alt.sh"), f"primary_mutant_{tag}", "-DPT_BUILD_EXPERIMENTS=1", f"-D{macro}={n}"],
                              env=dict(os.environ, ALT_SRCS=srcs, ALT_LIB="libptcore_lab.so")) for tag, macro, n, _ in MUTANTS]
    if any(p.wait() for p in procs):
        sys.exit("a mutant library did not build")


def run_one(tag):
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["PT_LIB_OVERRIDE"] = lib_of(tag)
    import numpy as np
    import __graft_entry__ as ge
    import footprint_cases, footprint_model, primlist_cases, primlist_model
    lab = ge.load_package()
    lab.set_device(0)
    kw = next(m[3] for m in MUTANTS if m[0] == tag)
    out = {"mutant": tag, "constant": kw, "fingerprint": lab.build_fingerprint(), "cases": []}
    if tag[0] == "f":
        for seed in (12,) + footprint_cases.EXTRA_SEEDS:
            sc, eye, basis, size, rb, re_, _ = footprint_cases.case(lab, seed)
            got = lab.primary_masks(sc, eye, basis, size, size, rb, re_)
            sound = footprint_model.primary_candidates(sc, eye, basis, size, size, rb, re_)["word"]
            same = footprint_model.primary_candidates(sc, eye, basis, size, size, rb, re_, **kw)["word"]
            out["cases"].append({"case": seed, "pixels": int(got.size), "differ_from_sound_model": int((got != sound).sum()),
                                 "differ_from_mutant_model": int((got != same).sum())})
    else:
        for name, sc, eye, basis, w, h, rb, re_ in primlist_cases.random_cases(lab, counts=(300,)):
            hdr, lists = lab.primary_lists(sc, eye, basis, w, h, rb, re_, threads=512)
            args = (sc, eye, basis, w, h, rb, re_, 512, *(float(x) for x in hdr[16:18].view(np.float32)), int(hdr[18]))
            sound = primlist_model.build_primary_lists(*args)["words"]
            same = primlist_model.build_primary_lists(*args, **kw)["words"]
            out["cases"].append({"case": name, "lanes": int(len(lists)), "differ_from_sound_model": int((lists != sound).any(axis=1).sum()),
                                 "differ_from_mutant_model": int((lists != same).any(axis=1).sum())})
    out["caught"] = sum(c["differ_from_sound_model"] for c in out["cases"]) > 0
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1:] == ["build"]:
        build()
    elif sys.argv[1:] == ["run"]:
        for tag, *_ in MUTANTS:  # (a library that fails to run ends the tool: nothing more is started on the device after it)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "run_one", tag], timeout=120)
            if rc:
                sys.exit(f"mutant {tag}: exit status {rc}")
    elif len(sys.argv) == 3 and sys.argv[1] == "run_one":
        run_one(sys.argv[2])
    else:
        sys.exit(__doc__)
