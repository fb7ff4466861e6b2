"""The builds of the pixel kernels and the case table of tests/test_kernel_census_gpu.py, without a device.

The lab library lists every kernel function its selectors can return (pt_debug_kernel_builds: found by walking select_kernel and
the fast mode's selector) and the rows of the variant table (pt_debug_variant_row).  Here:

  * the rule by which a row announces builds (csrc/pt_kernel.hip, variant_kernel) is restated over the exported rows and compared
    with that list as sets -- a build a row announces but the selector answers null for fails here, not as hipErrorInvalidValue
    at somebody's launch -- and its product subset with the variants the product library accepts;
  * the counts are printed and held to the restated rule;
  * the GPU file's case table must declare every build of the lab library, and its product cases every product build;
  * for every build, the cases that declare it must between them take every run-time arm that is applicable to it
    (applicable_arms below: written once, with the source line that makes each arm exist)."""
import ctypes

import test_kernel_census_gpu as tc
from test_kernel_census_gpu import ADAPTIVE, CASES, FAST, FAST_ROW, FRAMES, PLAIN, RESUME, Build

LEAN_NEVER, LEAN_BIG, LEAN_ALWAYS = 0, 1, 2  # csrc/pt_kernel.h, PT_LEAN_*


def announced_builds(rows, lab_library):
    """variant_kernel's rule: the builds a library holds, from the rows alone."""
    out = set()
    for r in rows:
        if not (r["product"] or lab_library):
            continue  # `if constexpr ((v.product || PT_BUILD_EXPERIMENTS) && ...`
        for rng in (0, 1):
            for flavour in (PLAIN, FRAMES, RESUME, ADAPTIVE):
                if flavour in (RESUME, ADAPTIVE) and not r["resume"]:
                    continue  # `(!RESUME || v.resume)`
                if flavour == FRAMES and not r["frames"]:
                    continue  # `(!FRAMES || v.frames)`
                if r["ref_builds"] and r["lean"] != LEAN_ALWAYS:  # `if (ref == 5 && !lean) ...; if (ref == 8 && !lean) ...`
                    out |= {Build(flavour, rng, r["kernel"], r["wide"], 0, ref) for ref in (5, 8)}
                if flavour == FRAMES:
                    continue  # `if constexpr (!FRAMES)`: a batch has builds for the reference configurations only
                if r["lean"] != LEAN_NEVER:
                    out.add(Build(flavour, rng, r["kernel"], r["wide"], 1, 0))
                if r["lean"] != LEAN_ALWAYS:
                    out.add(Build(flavour, rng, r["kernel"], r["wide"], 0, 0))
    for rng in (0, 1):  # csrc/pt_fast.hip, select_fast: <9, 5> and the generic build, in both libraries
        out |= {Build(FAST, rng, FAST_ROW, 0, 0, 5), Build(FAST, rng, FAST_ROW, 0, 0, 0)}
    return out


def launch_row(build, rows):
    """The table row a launch of this build is made as (a wide build: the wide row that names its kernel)."""
    if build.flavour == FAST:
        return None
    for r in rows:
        if r["kernel"] == build.kernel and r["wide"] == build.wide and (build.wide or rows.index(r) == build.kernel):
            return r
    raise AssertionError(f"no row launches {build}")


def applicable_arms(build, rows):
    """The run-time arms INSIDE a build that its cases must take between them.  Priority and repair are recorded by the census
    but not required: priority changes no value, repair is tests/test_chunk_chain_gpu.py's.  The fast builds' own arms (planar
    store, vertices, the masked ranking from 8 spp) are held by tests/test_fast_rays_gpu.py, test_fast_nearest_gpu.py and
    test_parity_gpu.py against their own references: here a fast build must be launched and held to the model, no more."""
    arms = set()
    if build.flavour == FAST:
        return arms
    r = launch_row(build, rows)
    # pt_kernel.hip, pixel_kernel: `constexpr bool CHUNKS = K.chunk_build(REF) && !FRAMES && !RESUME;` (pixel_kernel_split:
    # `K.chunk_build(REF)`), and the launcher chunks only rows that can (pt_kernel_chunked reads the LAUNCH row: 14 cannot)
    if build.flavour == PLAIN and r["can_chunk"] and (not r["ref_builds"] or build.ref):
        arms |= {"chunked", "unchunked"}
    # pixel_kernel: `} else if (!REF && a.planar) {` after `if (ADAPTIVE) {` (an adaptive pass stores no frame);
    # pixel_kernel_split: `const bool planar = !REF && a.planar;`
    if build.ref == 0 and build.flavour in (PLAIN, RESUME):
        arms |= {"planar", "interleaved"}
    # pt_capi.hip: fill_args `a->vertices = r->d_vertices;` (plain and batch launches); progressive_args `a.vertices = nullptr;`
    if build.flavour in (PLAIN, FRAMES):
        arms |= {"vertices", "no_vertices"}
    # pixel_kernel / pixel_kernel_split: `if (a.rng_state && active) {` ... `} else { xorwow_init(...)`, XORWOW builds; a batch
    # without persisted state never reaches the frames kernel (pt_renderer_enqueue_frames: `r->d_state != nullptr`)
    if build.flavour == PLAIN and build.rng == 0:
        arms |= {"fresh", "persisted"}
    # pixel_kernel: `if constexpr (REF) { ... if (pass_spp >= PT_FOOTPRINT_MIN_SPP) {`; pixel_kernel_split: `a.spp >= ...`
    if build.ref:
        arms |= {"footprint", "no_footprint"}
    # pixel_kernel: `if (sample_begin > 0 && active) {  // the session's record`
    if build.flavour in (RESUME, ADAPTIVE):
        arms |= {"first_pass", "later_pass"}
    return arms


def observed_arms(case, modes):
    """The arms a case took, from the mode bits the census reported for it (the GPU file's summary uses this)."""
    b = case.build
    arms = set()
    if b.flavour in (RESUME, ADAPTIVE):
        arms |= {"first_pass"} if modes & tc.M_FIRST_PASS else set()
        arms |= {"later_pass"} if len(case.passes) > 1 else set()
        arms |= {"footprint"} if modes & tc.M_FOOTPRINT else set()
        arms |= {"no_footprint"} if b.ref and min(case.passes) < tc.FOOTPRINT_MIN_SPP else set()
    else:
        arms.add("chunked" if modes & tc.M_CHUNKED else "unchunked")
        arms.add("vertices" if modes & tc.M_VERTICES else "no_vertices")
        arms.add("persisted" if modes & tc.M_RNG_STATE else "fresh")
        if b.ref:
            arms.add("footprint" if modes & tc.M_FOOTPRINT else "no_footprint")
    arms.add("planar" if modes & tc.M_PLANAR else "interleaved")
    return arms


def lab_builds(lab):
    return [Build(b["flavour"], b["rng"], b["kernel"], b["wide"], b["lean"], b["ref"]) for b in lab.kernel_builds()]


def product_variants(pt):
    """The rows the product library accepts, without a device: pt_renderer_create refuses a row that is not in the build before
    it touches one (PT_EINVAL, "... is not in this build"); any other answer, success or a device error, means it is there."""
    have = []
    for v in range(32):
        o = pt.RendererOpts()
        pt.lib.pt_renderer_opts_default(ctypes.byref(o))
        o.variant = v
        h = ctypes.c_void_p()
        rc = pt.lib.pt_renderer_create(8, 8, 1, 8, ctypes.byref(o), ctypes.byref(h))
        if rc == 0:
            pt.lib.pt_renderer_destroy(h)
        if not (rc == -1 and b"is not in this build" in pt.lib.pt_last_error()):
            have.append(v)
    return have


def test_the_enumeration_is_what_the_rows_announce(pt, lab):
    rows = lab.variant_rows()
    assert len(rows) == 15 and all(rows[r["kernel"]]["kernel"] == r["kernel"] for r in rows)
    listed = lab_builds(lab)
    assert len(set(listed)) == len(listed), "two builds with the same description"
    want = announced_builds(rows, True)
    assert set(listed) == want, f"announced but not selectable: {sorted(want - set(listed))}; selectable but not announced: {sorted(set(listed) - want)}"
    for b, x in zip(listed, lab.kernel_builds()):  # lanes per pixel, and the first row that selects the build
        if b.flavour != FAST:
            assert x["lanes"] == launch_row(b, rows)["lanes"] and rows[x["row"]] == launch_row(b, rows)
    assert [i for i, r in enumerate(rows) if r["product"]] == product_variants(pt)
    assert product_variants(lab) == list(range(15))
    assert announced_builds(rows, False) <= set(listed)


def test_build_counts(lab):
    rows = lab.variant_rows()
    n_lab, n_product = len(lab_builds(lab)), len(announced_builds(rows, False))
    print(f"builds: {n_lab} in the lab library, {n_product} of them in the product library")
    assert n_lab == len(announced_builds(rows, True)) and n_product < n_lab
    # the same rule, counted: per generator and row, (2 reference configurations + the layouts) per flavour it has, + the fast mode's 4
    def count(lab_library):
        n = 4
        for r in rows:
            if r["product"] or lab_library:
                refs = 2 if r["ref_builds"] and r["lean"] != LEAN_ALWAYS else 0
                layouts = 2 if r["lean"] == LEAN_BIG else 1
                n += 2 * ((refs + layouts) * (1 + 2 * r["resume"]) + refs * r["frames"])
        return n
    assert (n_lab, n_product) == (count(True), count(False))


def test_the_case_table_declares_every_build(lab):
    rows = lab.variant_rows()
    declared = {c.build for c in CASES}
    every = set(lab_builds(lab))
    assert declared <= every, f"cases for builds that do not exist: {sorted(declared - every)}"
    assert every <= declared, f"builds without a case: {sorted(every - declared)}"
    # the product cases are the cases of product builds (the GPU test runs exactly those again under libptcore.so)
    product = announced_builds(rows, False)
    assert product <= {c.build for c in CASES if c.build in product}
    for c in CASES:  # a declared row is one whose launches can be this build
        if c.build.flavour != FAST:
            assert rows[c.row]["kernel"] == c.build.kernel or (c.row == 12 and c.mb < 1 and c.build.kernel == 11), c.id
            assert rows[c.row]["wide"] == c.build.wide, c.id
            assert c.build.lean == (rows[c.row]["lean"] == LEAN_ALWAYS or (rows[c.row]["lean"] == LEAN_BIG and tc.SCENE_SPHERES[c.scene] > 10)), c.id
            ref = c.mb if (tc.SCENE_SPHERES[c.scene] == 9 and c.mb in (5, 8) and not c.planar and rows[c.row]["ref_builds"]) else 0
            assert c.build.ref == ref, c.id


def test_every_applicable_arm_is_declared_for_every_build(lab):
    rows = lab.variant_rows()
    missing = {}
    for b in lab_builds(lab):
        took = set().union(*(tc.arms_of(c) for c in CASES if c.build == b))
        lack = applicable_arms(b, rows) - took
        if lack:
            missing[tuple(b)] = sorted(lack)
    assert not missing, missing
    for c in CASES:  # a case that asks for chunks sits on a build that chunks, at a count pt_kernel_chunked accepts
        if c.chunks:
            assert "chunked" in applicable_arms(c.build, rows) and tc.chunked_by_rule(c), c.id
        assert observed_arms(c, tc.modes_of(c)) == tc.arms_of(c), c.id  # (the two readings of a case's arms agree)
