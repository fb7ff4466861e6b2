"""The two primary-ray exclusion analyses (csrc/pt_footprint.h, csrc/pt_primlist.h) as NumPy models, held to the reference's own
intersection (tests/numpy_restatement.intersect_scene) on the CPU: a sphere that a model leaves out is never the one the
reference returns, for any jitter a pixel can draw.  tests/test_primary_exclusion_gpu.py then requires the device to equal the
models bit for bit, so soundness shown here is soundness of the kernels.

Directions.  Every pixel gets a 5 x 5 lattice of jitter values whose ends are the two extreme values the project's uniform can
return (footprint_model.UNIFORM_MIN / UNIFORM_MAX, from uniform_from_u32's definition).  Every pixel with a (pixel, sphere) pair
NEAR a rule's threshold also gets 18 x 18; "near" is computed from the model's own quantities (footprint_model.NEAR_RHO = 4
footprint radii for the silhouette rule (A) and the behind rule (B), NEAR_C = a factor 1.2 between the two sides of (C)).

The primary lists are checked per sphere in the same way (second half of this file): whatever a lane's own cone leaves out is
never hit by the reference's single-sphere intersection on the lattice; the promise derived from rule (M); both mutants'
constants; every arm and the three constructed fallbacks.

Power.  The same check FAILS with the two constants of the deliberately unsound builds (PT_FOOTPRINT_MUTANT): margin 0.93 on at
least 10 of the 16 base cases, radius factor 0.3 on case 12 in at least 5 pixels."""
import functools

import numpy as np
import pytest

import footprint_model as fm
import primlist_cases as pc
import primlist_model as pm
from footprint_cases import BASE_SEEDS, EXTRA_SEEDS, case
from numpy_restatement import intersect_scene

f32, f64 = np.float32, np.float64
SIZE = 256
ARMS_FLOOR = 20  # the project's floor of occurrences per arm


def lattice(n):
    v = np.linspace(float(fm.UNIFORM_MIN), float(fm.UNIFORM_MAX), n).astype(f32)
    v[0], v[-1] = fm.UNIFORM_MIN, fm.UNIFORM_MAX
    return v


def reference_hits(spheres, eye, basis, size, row, col, n_lat):
    """int8 [n_lat * n_lat][pixels]: the sphere the reference returns for each lattice jitter of each pixel, -1 for a miss"""
    lat = lattice(n_lat)
    out = np.empty((n_lat * n_lat, row.size), dtype=np.int8)
    o = [np.full(row.size, f32(eye[k]), dtype=f32) for k in range(3)]
    for a, jx in enumerate(lat):
        for b, jy in enumerate(lat):
            d = fm.jittered_dir(basis, size, size, row, col, np.full(row.size, jx, dtype=f32), np.full(row.size, jy, dtype=f32))
            hit, _, index = intersect_scene(o, d, spheres)
            out[a * n_lat + b] = np.where(hit, index, -1)
    return out


@functools.lru_cache(maxsize=None)
def _case_reference(seed, size):
    """Computed once per case and shared: the case, the sound model's result, the reference's hits on the 5 x 5 lattice of every
    pixel and on the 18 x 18 lattice of the near pixels."""
    import __graft_entry__ as ge

    sc, eye, basis, size, rb, re_, _ = case(ge.load_package(), seed, size)
    row, col = fm.tile_pixels(size, rb, re_)
    model = fm.primary_candidates(sc, eye, basis, size, size, rb, re_)
    near = np.nonzero(model["near"])[0]
    return {"case": (sc, eye, basis, size, rb, re_), "model": model, "hits5": reference_hits(sc, eye, basis, size, row, col, 5),
            "near": near, "hits18": reference_hits(sc, eye, basis, size, row[near], col[near], 18)}


def wrong_pixels(ref, word):
    """Tile pixels where some lattice direction's reference hit is a sphere the word leaves out"""
    def missing(hits, w):
        h = hits.astype(np.int64)
        return ((h >= 0) & (((w[None, :] >> np.maximum(h, 0).astype(np.uint32)) & np.uint32(1)) == 0)).any(axis=0)
    bad = missing(ref["hits5"], word)
    bad[ref["near"]] |= missing(ref["hits18"], word[ref["near"]])
    return np.nonzero(bad)[0]


def mutant_word(ref, **kw):
    sc, eye, basis, size, rb, re_ = ref["case"]
    return fm.primary_candidates(sc, eye, basis, size, size, rb, re_, **kw)["word"]


@pytest.mark.parametrize("seed", BASE_SEEDS + EXTRA_SEEDS)
def test_footprint_model_is_sound(seed):
    ref = _case_reference(seed, SIZE)
    bad = wrong_pixels(ref, ref["model"]["word"])
    rays = ref["hits5"].size + ref["hits18"].size
    print(f"case {seed}: {rays} rays, {len(ref['near'])} near pixels, {len(bad)} wrong pixels")
    assert len(bad) == 0, (seed, bad[:8], ref["model"]["word"][bad[:8]])


def test_footprint_margin_mutant_is_noticed():
    failing = [seed for seed in BASE_SEEDS if len(wrong_pixels(_case_reference(seed, SIZE), mutant_word(_case_reference(seed, SIZE), margin=0.93)))]
    print(f"margin 0.93 fails cases {failing}")
    assert len(failing) >= 10, failing


@pytest.mark.parametrize("seed", (12,) + EXTRA_SEEDS)
def test_footprint_radius_mutant_is_noticed(seed):
    ref = _case_reference(seed, SIZE)
    bad = wrong_pixels(ref, mutant_word(ref, radius_factor=0.3))
    print(f"radius factor 0.3, case {seed}: {len(bad)} wrong pixels")
    assert len(bad) >= 5, (seed, len(bad))


def test_footprint_arms():
    """Over the committed cases each arm occurs at least ARMS_FLOOR times: the four drop rules, keep-all by a coarse footprint
    (the 64-pixel image of the device test, modelled here), keep-all by n."""
    import __graft_entry__ as ge

    pt = ge.load_package()
    count = {"A": 0, "B": 0, "C_out": 0, "C_wall": 0, "coarse": 0, "by_n": 0}
    for seed in BASE_SEEDS + EXTRA_SEEDS:
        sc, eye, basis, size, rb, re_, _ = case(pt, seed, SIZE)
        m = fm.primary_candidates(sc, eye, basis, size, size, rb, re_)
        for k in ("A", "B", "C_out", "C_wall"):
            count[k] += int((m[k] != 0).sum())
    sc, eye, basis, size, rb, re_, _ = case(pt, 0, 64)
    count["coarse"] = int(fm.primary_candidates(sc, eye, basis, 64, 64, 0, 64)["keep_all_coarse"].sum())
    for n in (1, 17):
        m = fm.primary_candidates(np.concatenate([sc, sc])[:n], eye, basis, 64, 64, 0, 64)
        assert m["keep_all_n"] and (m["word"] == (1 << n) - 1).all()
        count["by_n"] += m["word"].size
    print(count)
    assert min(count.values()) >= ARMS_FLOOR, count


# ---- not tests: the seed search and the bisection whose results are recorded in footprint_cases.EXTRA_SEEDS and EXACTNESS.md A.7 ----
def search_seeds(first, count, size=SIZE):
    """[(seed, wrong pixels with radius factor 0.3, wrong pixels of the sound model)] for seeds first .. first + count - 1"""
    out = []
    for seed in range(first, first + count):
        ref = _case_reference(seed, size)
        out.append((seed, len(wrong_pixels(ref, mutant_word(ref, radius_factor=0.3))), len(wrong_pixels(ref, ref["model"]["word"]))))
        _case_reference.cache_clear()
    return out


def critical_value(seeds, name, sound, unsound, steps=12, size=SIZE):
    """Bisection between a sound and an unsound value of radius_factor / margin: the value closest to `sound` at which the case
    set was still seen unsound, and the one next to it that was sound."""
    refs = [_case_reference(s, size) for s in seeds]
    for _ in range(steps):
        mid = 0.5 * (sound + unsound)
        if any(len(wrong_pixels(r, mutant_word(r, **{name: mid}))) for r in refs):
            unsound = mid
        else:
            sound = mid
    return unsound, sound


# ---- the primary lists (csrc/pt_primlist.h) ------------------------------------------------------------------------------------------
# Pairs (pixel, sphere) are handed to the reference's intersection unless the centre lies farther from the line through the pixel's
# centre direction than r + PREFILTER_RHO footprint radii * |off| + 1e-3 |off|: twenty times the cone the analysis itself uses,
# where the reference's float discriminant (relative error 2^-20) cannot be positive.  It only keeps the test's cost finite.
PREFILTER_RHO = 20.0


def _pkg():
    import __graft_entry__ as ge

    return ge.load_package()


def _line_distance(spheres, eye, d):
    """float64 [pixels][n]: distance of every centre from the line through the eye along d (d: [3][pixels] float32), |off| [n]"""
    off = np.asarray([f64(f32(eye[k])) for k in range(3)])[None, :] - spheres["pos"].astype(f64)
    dd = np.stack([x.astype(f64) for x in d], axis=1)
    dd /= np.linalg.norm(dd, axis=1)[:, None]
    h = dd @ off.T
    o2 = (off * off).sum(axis=1)
    return np.sqrt(np.maximum(o2[None, :] - h * h, 0.0)), np.sqrt(o2)



def list_violations(spheres, eye, basis, width, height, rb, re_, model, n_lat=5):
    """(pixel, sphere) pairs where the reference's single-sphere intersection HITS a sphere that a lane's own cone leaves out, over the
    jitter lattice of every pixel whose lane got as far as its own cone; and the number of rays tested"""
    px = model["pixels"]
    valid = model["analysed"][:px]  # (per sphere: also where more than five are kept and the list is given up)
    row, col = fm.tile_pixels(width, rb, re_)
    d5 = fm.five_dirs(basis, width, height, row, col)
    p_c, lo = _line_distance(spheres, eye, d5[0])
    rho = model["rho"][:px].astype(f64)
    cand = valid[:, None] & ~model["members"][:px] & (p_c <= spheres["radius"].astype(f64)[None, :] + (PREFILTER_RHO * rho[:, None] + 1e-3) * lo[None, :])
    pi, si = np.nonzero(cand)
    bad = np.zeros(pi.size, dtype=bool)
    lat = lattice(n_lat)
    o = [np.full(pi.size, f32(eye[k]), dtype=f32) for k in range(3)]
    one = [{"pos": [spheres["pos"][si, k] for k in range(3)], "radius": spheres["radius"][si]}]
    for jx in lat:
        for jy in lat:
            d = fm.jittered_dir(basis, width, height, row[pi], col[pi], np.full(pi.size, jx, dtype=f32), np.full(pi.size, jy, dtype=f32))
            hit, _, _ = intersect_scene(o, d, one)
            bad |= hit
    return list(zip(pi[bad].tolist(), si[bad].tolist())), pi.size * n_lat * n_lat


def host_model(spheres, eye, basis, width, height, rb, re_, threads=512, **kw):
    """every sphere a grid sphere (r_small = 0, r_big = inf): soundness is per sphere, as EXACTNESS.md A.13 claims"""
    return pm.build_primary_lists(spheres, eye, basis, width, height, rb, re_, threads, 0.0, np.inf, 4000, **kw)


@functools.lru_cache(maxsize=None)
def _list_cases():
    return pc.random_cases(_pkg())


@pytest.mark.parametrize("i", range(18))
def test_primary_list_model_is_sound_and_keeps_its_promise(i):
    name, sc, eye, basis, w, h, rb, re_ = _list_cases()[i]
    m = host_model(sc, eye, basis, w, h, rb, re_)
    bad, rays = list_violations(sc, eye, basis, w, h, rb, re_, m)
    px = m["pixels"]
    valid = m["words"][:px, 0] == 1
    print(f"{name}: {int(valid.sum())} of {px} pixels have lists, {rays} rays, {len(bad)} violations")
    assert not bad, (name, bad[:8])
    # the promise, from rule (M) as written: with rho in float64 from the corner directions, a sphere whose centre is farther from
    # the centre line than 1.01 rho |off| + sqrt(rr + 2^-17 o2) is on no valid list
    row, col = fm.tile_pixels(w, rb, re_)
    d5 = [[x.astype(f64) for x in d] for d in fm.five_dirs(basis, w, h, row, col)]
    lc = np.sqrt(sum(x * x for x in d5[0]))
    dev = np.max([np.sqrt(sum((d5[1 + k][a] - d5[0][a]) ** 2 for a in range(3))) for k in range(4)], axis=0)
    rho = 1.05 * dev / lc + 1e-6
    p_c, lo = _line_distance(sc, eye, fm.five_dirs(basis, w, h, row, col)[0])
    rr = sc["radius"].astype(f64) ** 2
    far = p_c > 1.01 * rho[:, None] * lo[None, :] + np.sqrt(rr + 2.0 ** -17 * lo * lo)[None, :]
    listed_far = m["members"][:px] & far & m["analysed"][:px, None]
    assert not listed_far.any(), (name, np.argwhere(listed_far)[:8])


@pytest.mark.parametrize("kw", [{"miss_scale": 0.64}, {"radius_factor": 0.3}], ids=["miss_scale_0.64", "radius_factor_0.3"])
def test_primary_list_mutants_are_noticed(kw):
    found = 0
    for name, sc, eye, basis, w, h, rb, re_ in _list_cases()[:6]:
        bad, _ = list_violations(sc, eye, basis, w, h, rb, re_, host_model(sc, eye, basis, w, h, rb, re_, **kw))
        found += len(bad)
    print(f"{kw}: {found} (pixel, sphere) violations")
    assert found > 0


def coarse_cases(pt):
    """4 x 4 images from two eyes: every pixel's own cone is wider than 0.125 rad (rho = 0.13 .. 0.15)"""
    sc = pt.scene_random(72, seed=2, with_walls=False)
    return [(f"coarse_4px_{i}", sc, eye, pt.camera_basis(eye, -90.0, 0.0, 4, 4), 4, 4, 0, 4) for i, eye in enumerate((pc.DEFAULT_EYE, (40.0, 30.0, 200.0)))]


def list_arms(results):
    """Occurrences of every arm of build_primary_list over [(words [lanes][6], model)]: the words may be the model's own or the
    device's (the reasons a lane has no list are the model's: the device reports only that it has none)"""
    arms = dict.fromkeys(("k0", "k1_3", "k4_5", "drop_M", "drop_B", "list_long", "survivors", "wave_wide", "cone_wide", "inactive"), 0)
    for words, m in results:
        ok, k = words[:, 0] == 1, words[:, 1]
        arms["k0"] += int((ok & (k == 0)).sum())
        arms["k1_3"] += int((ok & (k >= 1) & (k <= 3)).sum())
        arms["k4_5"] += int((ok & (k >= 4)).sum())
        arms["drop_M"] += m["drop_M"]
        arms["drop_B"] += m["drop_B"]
        for name, why in (("list_long", pm.LIST_LONG), ("survivors", pm.SURVIVORS), ("wave_wide", pm.WAVE_WIDE), ("cone_wide", pm.CONE_NAN_OR_WIDE),
                          ("inactive", pm.INACTIVE)):
            arms[name] += int(((words[:, 0] == 0) & (m["why"] == why)).sum())
    return arms


def test_primary_list_arms_and_fallbacks():
    pt = _pkg()
    results = []
    for name, sc, eye, basis, w, h, rb, re_ in _list_cases() + coarse_cases(pt):
        m = host_model(sc, eye, basis, w, h, rb, re_)
        results.append((m["words"], m))
    for name, sc, eye, basis, w, h, rb, re_, (kind, where) in pc.fallback_cases(pt):
        m = host_model(sc, eye, basis, w, h, rb, re_)
        results.append((m["words"], m))
        why, px = m["why"], m["pixels"]
        if kind == "pixel":  # the pixel on the line has no list, nor have the few around it whose cones (footprint + rule (M)'s
            # own slack of 2.2 mrad + the spheres' 4-8 mrad, at 2.5 mrad per pixel) still reach all six; eight columns away the lists are back
            assert why[where] == pm.LIST_LONG, (name, why[where])
            assert (why[[where - 8, where + 8]] == pm.VALID).all(), name
            assert (why[:px] == pm.LIST_LONG).sum() <= 40, (name, int((why[:px] == pm.LIST_LONG).sum()))
        elif kind == "wave":  # the wave over the strip gives up; the waves beside it in its row do not (a pixel at the
            # strip's edge may still see more than five)
            assert (why[64 * where:64 * where + 64] == pm.SURVIVORS).all(), name
            beside = np.concatenate([why[64 * (where - 1):64 * where], why[64 * (where + 1):64 * (where + 2)]])
            assert (beside != pm.SURVIVORS).all() and (beside == pm.VALID).sum() >= 96, name
        else:  # exactly the waves that hold pixels of two rows
            lane = np.arange(m["lanes"])
            wraps = np.zeros(m["lanes"], dtype=bool)
            for w0 in range(0, px, 64):
                last = min(w0 + 63, px - 1)
                wraps[w0:w0 + 64] = (w0 // w) != (last // w)
            assert ((why == pm.WAVE_WIDE) == (wraps & (lane < px))).all(), name
            assert (why[(lane < px) & ~wraps] == pm.VALID).all(), name
    arms = list_arms(results)
    print(arms)
    assert min(arms.values()) >= ARMS_FLOOR, arms
