"""Every build of the pixel kernels against the oracle, with the launch census as the proof of WHICH build was compared.

The libraries hold many compiled builds of the pixel kernel (csrc/pt_kernel.hip: kVariants and select_kernel; csrc/pt_fast.hip:
select_fast) -- 88 in the lab library, 72 of them in the product library.  A parity test says something about a build only if it
launches that build, and which one a renderer launches depends on the scene's size, the bounce cap, the layout, the tile and what
the cost model answers on the card at hand.  So every case below DECLARES the build it means (CASES, importable without a
device: tests/test_kernel_census_host.py checks that the table leaves out no build and no run-time arm of one), and the test

  1. resets the lab library's launch census (include/ptcore_lab.h, pt_debug_launch_census),
  2. renders through the public API, comparing all 14 channels with the oracle bit for bit after every frame and every pass
     (and the XORWOW state, the display vertices, every pixel of an adaptive session at its own count),
  3. asserts that exactly the declared build has launches, the declared number of them, with the declared mode bits,
  4. if the build is in the product library: runs the case again there (same bits, and the renderer reports the row).

The fast builds are toleranced, not exact: their cases are held to the float64 model by the checks of tests/test_fast_rays_gpu.py.

Shapes: 72 x 40 -- 11.25 workgroups of 256 threads, 5.6 of 512, 2.8 of 1024 (the last one ragged), waves straddle rows; one
case per flavour on rows 7..33 of it.  9 spp is past the footprint threshold (PT_FOOTPRINT_MIN_SPP = 8), odd and a multiple of
neither 2 nor 4 lanes; 3 spp is below it.  chunks = 4 at 9 spp: pt_kernel_chunked wants spp >= 2 chunks, 9 >= 8.  (The split
kernels round a chunk to whole rounds of their lanes: 4 samples each, so the chunks are [0,4) [4,8) [8,9) and an EMPTY fourth
one, which still has to hand the state on and write the frame.)  Sessions run the passes [3, 1, 5]; a resume build compares
the PASS's own count with the footprint threshold (pt_kernel.hip: pass_spp), not the session's, so the third pass (n = 9) does
not reach the analysis: the reference-configuration builds get a fourth pass of 8 samples that does."""
from collections import namedtuple

import numpy as np
import pytest

import fast_model as fm
from test_adaptive_gpu import _forced_masks, check_pixels_at_counts, download_frame, run_adaptive, tolerance_for
from test_fast_rays_gpu import _hold as fast_hold
from test_fast_rays_gpu import _render as fast_render
from test_frames_gpu import reference as frames_reference
from test_parity_gpu import assert_bit_exact

pytestmark = pytest.mark.gpu

W, H = 72, 40
TILE = (7, 33)
PLAIN, FRAMES, RESUME, ADAPTIVE, FAST = range(5)
FLAVOURS = ("plain", "frames", "resume", "adaptive", "fast")
FAST_ROW = 100
M_CHUNKED, M_REPAIR, M_PLANAR, M_VERTICES, M_RNG_STATE, M_FOOTPRINT, M_FIRST_PASS, M_PRIO = (1 << k for k in range(8))
MODE_NAMES = ("chunked", "repair", "planar", "vertices", "rng_state", "footprint", "first_pass", "prio")
FOOTPRINT_MIN_SPP = 8  # csrc/pt_kernel.h, PT_FOOTPRINT_MIN_SPP
SESSION_PASSES, SESSION_PASSES_REF = (3, 1, 5), (3, 1, 5, 8)

SCENE_SPHERES = {"cornell": 9, "open6": 6, "closed40": 40, "open40": 40, "closed300": 300, "open300": 300}
FAST_CASES = {5: "cornell_41x67_b5", 0: "cornell_41x67_b8"}  # tests/fast_model.py: the <9, 5> build and the generic one


def scene_of(mod, name):
    if name == "cornell":
        return mod.scene_cornell()
    if name == "open6":  # the open subset of tests/test_parity_gpu.py::test_all_variants_bit_exact_vs_oracle: paths escape
        return mod.scene_cornell()[[0, 2, 4, 6, 7, 8]]
    return mod.scene_random(SCENE_SPHERES[name], 7, name.startswith("closed"))


# A build: (flavour, generator, kernel row, wide, lean, reference bounces) -- the first six words of pt_debug_kernel_builds.
Build = namedtuple("Build", "flavour rng kernel wide lean ref")
# A case.  row: the variant the renderer is forced to (the row kernel_info must report; FAST_ROW: a fast_math renderer).
# spp: samples of a plain render / of each frame of a batch; passes: a session's.  frames: renders (plain) or batch size.
Case = namedtuple("Case", "id build row scene mb spp frames passes persist planar vertices chunks tile")


def _case(flavour, rng, row, scene, mb, kernel, lean, ref, wide=0, spp=0, frames=1, passes=(), persist=True, planar=False,
          vertices=False, chunks=0, tile=None, tag=""):
    b = Build(flavour, rng, kernel, wide, lean, ref)
    what = f"spp{spp}" if not passes else "passes" + "_".join(map(str, passes))
    bits = [FLAVOURS[flavour], "xorwow" if rng == 0 else "philox", f"row{row}", scene, f"b{mb}", what]
    bits += [f"x{frames}"] if frames > 1 else []
    bits += ["fresh"] if flavour in (PLAIN, FRAMES) and rng == 0 and not persist else []
    bits += ["planar"] if planar else []
    bits += ["vtx"] if vertices else []
    bits += [f"chunks{chunks}"] if chunks else []
    bits += ["rows%d_%d" % tile] if tile else []
    bits += [tag] if tag else []
    return Case("-".join(bits), b, row, scene, mb, spp, frames, tuple(passes), persist, planar, vertices, chunks, tile)


def _build_cases():
    """The table, written from the rows of kVariants and the selector as they stand (csrc/pt_kernel.hip).  Per build two or three
    cases that between them take every run-time arm the build has (applicable_arms, tests/test_kernel_census_host.py)."""
    out = []
    for rng in (0, 1):
        # -- plain launches ---------------------------------------------------------------------------------------------------
        # generic builds with the scene in LDS: every one-lane row without a lean-only layout, and the split rows 8 and 9.
        # Cornell at 3 bounces is the nine-sphere screen without a reference configuration; the six-sphere subset is open.
        for row in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
            out.append(_case(PLAIN, rng, row, "cornell", 3, row, 0, 0, spp=9, frames=2))
            out.append(_case(PLAIN, rng, row, "open6", 5, row, 0, 0, spp=3, persist=False, planar=True, vertices=True))
        # the lean builds of rows 6, 8, 10 (above PT_SCREEN_MAX_SPHERES = 10 spheres), closed and open
        for row in (6, 8, 10):
            out.append(_case(PLAIN, rng, row, "closed40", 5, row, 1, 0, spp=9, frames=2))
            out.append(_case(PLAIN, rng, row, "open40", 5, row, 1, 0, spp=3, persist=False, planar=True, vertices=True))
        # the grid kernels: rows 11, 12, 13 and row 14 = kernel 13 in 1024-thread workgroups
        for row, kernel, wide in ((11, 11, 0), (12, 12, 0), (13, 13, 0), (14, 13, 1)):
            out.append(_case(PLAIN, rng, row, "closed300", 5, kernel, 1, 0, wide=wide, spp=9, frames=2))
            out.append(_case(PLAIN, rng, row, "open300", 5, kernel, 1, 0, wide=wide, spp=3, persist=False, planar=True, vertices=True))
        # row 13 chains samples through workgroups in every build (row 14, the same kernel, is never chunked by the host)
        out.append(_case(PLAIN, rng, 13, "closed300", 5, 13, 1, 0, spp=9, chunks=4))
        # the reference configurations (9 spheres, 5 or 8 bounces, interleaved) of rows 6, 8, 9: footprint on and off, fresh and
        # persisted generator, with and without vertices, chunked and not
        for row in (6, 8, 9):
            for mb in (5, 8):
                out.append(_case(PLAIN, rng, row, "cornell", mb, row, 0, mb, spp=9, frames=2))
                out.append(_case(PLAIN, rng, row, "cornell", mb, row, 0, mb, spp=3, persist=False, vertices=True))
                out.append(_case(PLAIN, rng, row, "cornell", mb, row, 0, mb, spp=9, chunks=4))
        # -- frame batches: the reference configurations of row 6 ------------------------------------------------------------
        for mb in (5, 8):
            out.append(_case(FRAMES, rng, 6, "cornell", mb, 6, 0, mb, spp=4, frames=3))
            out.append(_case(FRAMES, rng, 6, "cornell", mb, 6, 0, mb, spp=9, frames=2, vertices=True))
        # -- progressive sessions (resume builds) and adaptive ones (every pass of those is an adaptive launch: pt_capi.hip,
        #    launch_progressive_pass) -----------------------------------------------------------------------------------------
        for flavour in (RESUME, ADAPTIVE):
            for mb in (5, 8):
                out.append(_case(flavour, rng, 6, "cornell", mb, 6, 0, mb, passes=SESSION_PASSES_REF))
            for row, kernel, wide, small, closed, opened in ((6, 6, 0, True, "closed40", "open40"), (10, 10, 0, True, "closed40", "open40"),
                                                             (13, 13, 0, False, "closed300", "open300"), (14, 13, 1, False, "closed300", "open300")):
                if small:  # the builds with the scene in LDS: the nine-sphere screen and the generic one
                    out.append(_case(flavour, rng, row, "cornell", 3, kernel, 0, 0, passes=SESSION_PASSES))
                    out.append(_case(flavour, rng, row, "open6", 5, kernel, 0, 0, passes=SESSION_PASSES, planar=True))
                out.append(_case(flavour, rng, row, closed, 5, kernel, 1, 0, wide=wide, passes=SESSION_PASSES))
                out.append(_case(flavour, rng, row, opened, 5, kernel, 1, 0, wide=wide, passes=SESSION_PASSES, planar=True))
        # -- the fast mode: the reference's configuration as constants, and the generic build (8 bounces) ------------------------
        out.append(_case(FAST, rng, FAST_ROW, "cornell", 5, FAST_ROW, 0, 5, spp=1))
        out.append(_case(FAST, rng, FAST_ROW, "cornell", 8, FAST_ROW, 0, 0, spp=1))
    # one case per flavour on rows 7..33 of the frame (a ragged tile that starts and ends inside waves)
    out.append(_case(PLAIN, 0, 6, "cornell", 5, 6, 0, 5, spp=9, frames=2, tile=TILE))
    out.append(_case(FRAMES, 0, 6, "cornell", 5, 6, 0, 5, spp=4, frames=3, tile=TILE))
    out.append(_case(RESUME, 1, 6, "cornell", 8, 6, 0, 8, passes=SESSION_PASSES_REF, tile=TILE))
    out.append(_case(ADAPTIVE, 0, 6, "cornell", 5, 6, 0, 5, passes=SESSION_PASSES_REF, tile=TILE))
    out.append(_case(FAST, 0, FAST_ROW, "cornell", 5, FAST_ROW, 0, 5, spp=1, frames=2, tile=TILE, tag="tile_of_full"))
    # row 12's loop needs bounces: without any, the launcher runs row 11's kernel (pt_kernel.hip, run_variant)
    out.append(_case(PLAIN, 0, 12, "closed300", 0, 11, 1, 0, spp=3, tag="runs_row11"))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _build_cases()


def chunked_by_rule(case):
    """pt_kernel_chunked's arithmetic for a case whose build can chunk: 2 .. 16 chunks, spp >= 2 chunks, a chunk of at most 256
    (grid family) or 4096 samples."""
    c, spp = case.chunks, case.spp
    return 2 <= c <= 16 and spp >= 2 * c and (spp + c - 1) // c <= (256 if case.build.kernel == 13 else 4096)


def launches_of(case):
    """One launch per render, per group of <= 32 frames, per pass; a chunked launch is still one."""
    if case.build.flavour in (RESUME, ADAPTIVE):
        return len(case.passes)
    if case.build.flavour == FRAMES:
        return (case.frames + 31) // 32
    return case.frames


def modes_of(case):
    """The census bits of a case's launches, OR-ed (priority left out: it changes no value and depends on the chip's size)."""
    b = case.build
    m = 0
    if b.flavour in (RESUME, ADAPTIVE):
        m |= M_FIRST_PASS
        if b.ref and max(case.passes) >= FOOTPRINT_MIN_SPP:
            m |= M_FOOTPRINT
    else:
        if case.chunks > 1 and chunked_by_rule(case):
            m |= M_CHUNKED
        if case.vertices:
            m |= M_VERTICES
        if b.rng == 0 and case.persist:
            m |= M_RNG_STATE
        if b.ref and case.spp >= FOOTPRINT_MIN_SPP:
            m |= M_FOOTPRINT
    if case.planar:
        m |= M_PLANAR
    return m


def arms_of(case):
    """The run-time arms a case takes inside its build, by name (what the host test holds against applicable_arms)."""
    b, m = case.build, modes_of(case)
    arms = set()
    if b.flavour in (RESUME, ADAPTIVE):
        arms |= {"first_pass"} | ({"later_pass"} if len(case.passes) > 1 else set())
        if b.ref:
            arms |= {"footprint"} if m & M_FOOTPRINT else set()
            arms |= {"no_footprint"} if min(case.passes) < FOOTPRINT_MIN_SPP else set()
    else:
        arms.add("chunked" if m & M_CHUNKED else "unchunked")
        arms.add("vertices" if m & M_VERTICES else "no_vertices")
        arms.add("persisted" if m & M_RNG_STATE else "fresh")
        if b.ref:
            arms.add("footprint" if m & M_FOOTPRINT else "no_footprint")
    arms.add("planar" if m & M_PLANAR else "interleaved")
    return arms


def mode_names(m):
    return "+".join(n for k, n in enumerate(MODE_NAMES) if m >> k & 1) or "-"


# ---- the oracle, once per configuration ------------------------------------------------------------------------------------------
_ORACLE = {}


def _rows(case):
    return case.tile if case.tile else (0, H)


def oracle_renders(oracle, mod, case):
    """What `frames` Render() calls of a fresh renderer give: [(frame, XORWOW state afterwards or None)], read-only."""
    rb, re_ = _rows(case)
    key = ("plain", case.scene, case.mb, case.spp, case.build.rng, case.persist, rb, re_)
    got = _ORACLE.setdefault(key, {"frames": [], "st": None})
    carried = case.build.rng == 0 and case.persist
    while len(got["frames"]) < case.frames:
        f = len(got["frames"])
        if f == 0 and carried:
            got["st"] = oracle.setup_random(W, H, row_begin=rb, row_end=re_)
        img = oracle.render(W, H, case.spp, spheres=scene_of(mod, case.scene), basis=mod.camera_basis(width=W, height=H), max_bounces=case.mb,
                            rng_mode=case.build.rng, row_begin=rb, row_end=re_, rng_state=got["st"] if carried else None, frame=f)
        st = got["st"].copy() if carried else None
        for a in (img, st):
            if a is not None:
                a.setflags(write=False)
        got["frames"].append((img, st))
    return got["frames"][:case.frames]


def oracle_session(oracle, mod, case, n):
    """The first Render() of a fresh renderer at n spp (what a session holds after n samples; whole frame)."""
    key = ("session", case.scene, case.mb, n, case.build.rng)
    if key not in _ORACLE:
        img = oracle.render(W, H, n, spheres=scene_of(mod, case.scene), basis=mod.camera_basis(width=W, height=H), max_bounces=case.mb,
                            rng_mode=case.build.rng, frame=0)
        img.setflags(write=False)
        _ORACLE[key] = img
    return _ORACLE[key]


# ---- the runners: one per flavour, on `mod` (the lab or the product view) -----------------------------------------------------------
def _renderer(mod, case, spp, **kw):
    rb, re_ = _rows(case)
    r = mod.Renderer(W, H, spp, max_bounces=case.mb, rng_mode=case.build.rng, variant=None if case.row == FAST_ROW else case.row,
                     row_begin=rb if case.tile else 0, row_end=re_ if case.tile else 0,
                     layout=mod.LAYOUT_PLANAR if case.planar else mod.LAYOUT_INTERLEAVED, **kw)
    assert r.kernel_info(SCENE_SPHERES[case.scene])["variant"] == case.row, f"{case.id}: the renderer reports another row"
    return r


def run_plain(mod, oracle, case, tag):
    rb, re_ = _rows(case)
    rows = re_ - rb
    want = oracle_renders(oracle, mod, case)
    r = _renderer(mod, case, case.spp, persist_rng=case.persist, chunks=case.chunks)
    d_scene, ns = mod.upload_scene(scene_of(mod, case.scene))
    d_out, d_vtx = mod.DeviceBuffer(rows * W * 56), mod.DeviceBuffer(rows * W * 12)
    try:
        if case.chunks:
            lanes = {8: 4, 9: 2}.get(case.row, 1)
            blocks = (rows * W * lanes + r.kernel_info(ns)["block_threads"] - 1) // r.kernel_info(ns)["block_threads"]
            assert r.kernel_info(ns)["grid_blocks"] == blocks * case.chunks, f"{case.id}: the launch is not chunked"
        if case.vertices:
            r.set_display(d_vtx.ptr)
        for f, (ref, st) in enumerate(want):
            if case.vertices:
                d_vtx.upload(np.full((rows, W, 3), -3.0, dtype=np.float32))
            r.render(d_out.ptr, d_scene.ptr, ns, mod.camera_basis(width=W, height=H))
            assert_bit_exact(download_frame(d_out, rows, W, case.planar), ref, f"{tag} {case.id} frame {f}")
            if st is not None:
                assert np.array_equal(r.get_rng_state(), st), f"{tag} {case.id}: generator state after frame {f}"
            if case.vertices:
                assert not case.tile
                assert np.array_equal(d_vtx.download(np.float32, (rows, W, 3)).view(np.uint32), oracle.display_pack(ref).view(np.uint32)), \
                    f"{tag} {case.id}: display vertices of frame {f}"
    finally:
        r.destroy()
        for d in (d_scene, d_out, d_vtx):
            d.free()


def run_frames(mod, oracle, case, tag):
    rb, re_ = _rows(case)
    rows, n = re_ - rb, case.frames
    bases, eyes, frames, states = frames_reference(mod, oracle, (W, H), case.spp, case.build.rng, case.mb, n, rows=case.tile)
    r = _renderer(mod, case, case.spp)
    d_scene, ns = mod.upload_scene(scene_of(mod, case.scene))
    d_out, d_vtx = mod.DeviceBuffer(n * rows * W * 56), mod.DeviceBuffer(n * rows * W * 12)
    try:
        r.enqueue_frames(d_out.ptr, rows * W * 14, d_scene.ptr, ns, bases[:n], eyes[:n], d_vertices=d_vtx.ptr if case.vertices else None,
                         vtx_stride_floats=rows * W * 3 if case.vertices else 0)
        assert r.check(wait=True) == 0
        got = d_out.download(np.float32, (n, rows, W, 14))
        for f in range(n):
            assert_bit_exact(got[f], frames[f], f"{tag} {case.id} batched frame {f}")
        if case.build.rng == 0:
            assert np.array_equal(r.get_rng_state(), states[n]), f"{tag} {case.id}: generator state after the batch"
        if case.vertices:
            vtx = d_vtx.download(np.float32, (n, rows, W, 3))
            for f in range(n):
                assert not case.tile
                assert np.array_equal(vtx[f].view(np.uint32), oracle.display_pack(frames[f]).view(np.uint32)), f"{tag} {case.id}: vertices of frame {f}"
    finally:
        r.destroy()
        for d in (d_scene, d_out, d_vtx):
            d.free()


def run_resume(mod, oracle, case, tag):
    rb, re_ = _rows(case)
    rows = re_ - rb
    r = _renderer(mod, case, sum(case.passes))
    s = mod.Progressive(r)
    d_scene, ns = mod.upload_scene(scene_of(mod, case.scene))
    d_out = mod.DeviceBuffer(rows * W * 56)
    try:
        n = 0
        for k, p in enumerate(case.passes):
            assert s.variant(ns) == case.row
            s.render(p, d_out.ptr, d_scene.ptr, ns, mod.camera_basis(width=W, height=H))
            n += p
            assert s.samples() == n
            assert_bit_exact(download_frame(d_out, rows, W, case.planar), oracle_session(oracle, mod, case, n)[rb:re_], f"{tag} {case.id} pass {k} (n = {n})")
    finally:
        s.destroy()
        r.destroy()
        d_out.free()
        d_scene.free()


def _session_opts(mod, case):
    rb, re_ = _rows(case)
    return dict(variant=case.row, row_begin=rb if case.tile else 0, row_end=re_ if case.tile else 0,
                layout=mod.LAYOUT_PLANAR if case.planar else mod.LAYOUT_INTERLEAVED)


def run_adaptive_lab(lab, oracle, case, tag):
    """The forced sets of tests/test_adaptive_gpu.py: after the first pass (everyone) all pixels but one, then one pixel per wave
    in a different lane each (a forced set may only shrink), which the fourth pass of a reference configuration renders again.
    run_adaptive compares every pixel at its own count with the oracle after every pass, and the counts with the forced sets."""
    rb, re_ = _rows(case)
    masks = _forced_masks(re_ - rb, W)
    sparse = masks["one per wave"] & masks["all but one"]
    forced = {1: masks["all but one"], 2: sparse, 3: sparse}
    counts, ran = run_adaptive(lab, oracle, W, H, scene_of(lab, case.scene), list(case.passes), case.mb, case.build.rng,
                               ("census", case.scene), q=None, min_samples=4, forced={k: v for k, v in forced.items() if k < len(case.passes)},
                               **_session_opts(lab, case))
    assert ran == {case.row}
    assert (counts[sparse] == sum(case.passes)).all() and (counts[~masks["all but one"]] == case.passes[0]).all()


def run_adaptive_product(mod, oracle, case, tag):
    """The product library cannot force a set: the rule decides, with a tolerance that stops about half the pixels at the second
    pass's count (no dilation, so that they do stop).  Every pixel, at whatever count the session left it, is the oracle's pixel at that count."""
    rb, re_ = _rows(case)
    rows = re_ - rb
    r = _renderer(mod, case, 8)
    s = mod.Progressive(r)
    d_scene, ns = mod.upload_scene(scene_of(mod, case.scene))
    d_out = mod.DeviceBuffer(rows * W * 56)
    try:
        n_rule = case.passes[0] + case.passes[1]
        s.set_adaptive(tolerance_for(oracle_session(oracle, mod, case, n_rule)[rb:re_], n_rule, 0.05, 0.5), floor=0.05, min_samples=n_rule, radius=0)
        for k, p in enumerate(case.passes):
            assert s.variant(ns) == case.row
            s.render(p, d_out.ptr, d_scene.ptr, ns, mod.camera_basis(width=W, height=H))
            counts = s.counts().cpu().numpy().reshape(rows, W)
            check_pixels_at_counts(download_frame(d_out, rows, W, case.planar), counts, lambda n: oracle_session(oracle, mod, case, n)[rb:re_],
                                   f"{tag} {case.id} pass {k}")
        assert len(np.unique(counts)) >= 2, f"{case.id}: the rule stopped no pixel, or all of them, at once: {np.unique(counts)}"
    finally:
        s.destroy()
        r.destroy()
        d_out.free()
        d_scene.free()


_FAST = {}


def run_fast(mod, oracle, case, tag):
    """The checks of tests/test_fast_rays_gpu.py (strong on decided rays, weak on all, the case's cap on the undecided share)."""
    if "cases" not in _FAST:
        _FAST["cases"] = fm.cases(mod)
    fc = _FAST["cases"][FAST_CASES[case.build.ref]]
    assert fc.max_bounces == case.mb and fc.n == 9
    r = mod.Renderer(fc.width, fc.height, 1, fast_math=True, max_bounces=fc.max_bounces)
    assert r.kernel_info(fc.n)["variant"] == mod.VARIANT_FAST
    r.destroy()
    full = fast_render(mod, fc, rng_mode=case.build.rng)
    fast_hold(fc, full, f" {tag} rng {case.build.rng}")
    if case.tile:
        tile = fast_render(mod, fc, rng_mode=case.build.rng, row_begin=case.tile[0], row_end=case.tile[1])
        assert np.array_equal(tile.view(np.uint32), full.view(np.uint32)[case.tile[0]:case.tile[1]])


def run_case(mod, oracle, case, tag):
    f = case.build.flavour
    if f == ADAPTIVE:
        return (run_adaptive_lab if mod.IS_LAB else run_adaptive_product)(mod, oracle, case, tag)
    return {PLAIN: run_plain, FRAMES: run_frames, RESUME: run_resume, FAST: run_fast}[f](mod, oracle, case, tag)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
_SEEN = {}  # build -> [(case id, launches, modes)], as the census reported them: the summary at the end of the file


def census(lab):
    """{build: (launches, modes)} of the builds with launches since the reset, and the launches of functions in no build."""
    builds, counts = lab.kernel_builds(), lab.launch_census()
    got = {Build(b["flavour"], b["rng"], b["kernel"], b["wide"], b["lean"], b["ref"]): c for b, c in zip(builds, counts[:-1]) if c[0]}
    return got, counts[-1][0]


def product_builds(lab):
    rows = lab.variant_rows()
    product_rows = {r["kernel"] for r in rows if r["product"]} | {FAST_ROW}
    wide_product = any(r["product"] and r["wide"] for r in rows)
    return {b for b in (Build(x["flavour"], x["rng"], x["kernel"], x["wide"], x["lean"], x["ref"]) for x in lab.kernel_builds())
            if b.kernel in product_rows and (not b.wide or wide_product)}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_build_against_oracle_and_census(pt, lab, oracle, gpu, case):
    lab.launch_census_reset()
    run_case(lab, oracle, case, "lab")
    got, unknown = census(lab)
    line = {b: f"{n} launches, modes {mode_names(m)}" for b, (n, m) in got.items()}
    print(f"{case.id}: declared {tuple(case.build)} x {launches_of(case)} modes {mode_names(modes_of(case))}; census {line}")
    for b, (n, m) in got.items():
        _SEEN.setdefault(b, []).append((case.id, n, m))
    assert unknown == 0, f"{case.id}: {unknown} launches of a function that is in no build"
    assert {b: n for b, (n, m) in got.items()} == {case.build: launches_of(case)}, f"{case.id}: declared {tuple(case.build)}, launched {line}"
    assert got[case.build][1] & ~M_PRIO == modes_of(case), f"{case.id}: modes {mode_names(got[case.build][1])}, declared {mode_names(modes_of(case))}"
    if case.build in product_builds(lab):  # the same source compiled into the product library: same bits, and it reports the row
        run_case(pt, oracle, case, "product")


def test_summary_every_build_launched_with_every_applicable_arm(lab, gpu):
    """Runs after the cases (file order): every build of the lab library with the cases that launched it, and nothing missing."""
    from test_kernel_census_host import applicable_arms, observed_arms

    rows = lab.variant_rows()
    missing = []
    for x in lab.kernel_builds():
        b = Build(x["flavour"], x["rng"], x["kernel"], x["wide"], x["lean"], x["ref"])
        seen = _SEEN.get(b, [])
        print(f"{FLAVOURS[b.flavour]:8s} rng {b.rng} kernel {b.kernel:3d} wide {b.wide} lean {b.lean} ref {b.ref}: "
              + ("; ".join(f"{cid} x{n} [{mode_names(m)}]" for cid, n, m in seen) or "NO LAUNCH"))
        if not seen:
            missing.append((tuple(b), "no launch"))
            continue
        by_id = {c.id: c for c in CASES}
        lack = applicable_arms(b, rows) - set().union(*(observed_arms(by_id[cid], m) for cid, n, m in seen))
        if lack:
            missing.append((tuple(b), sorted(lack)))
    assert not missing, missing
