"""CPU tests of tests/fast_model.py, the float64 model every ray of the fast mode is held to (tests/test_fast_rays_gpu.py):

  * THE ORACLE AGAINST THE MODEL.  On every case of the GPU test the reference's CPU restatement, rendered at 1 spp, must pass
    the checks the kernel is held to: strong on decided rays, weak on all, the undecided share under the case's cap.  The
    reference decides hit or miss with a float b*b - 4ac and forms its t in double from float a, b, c -- the same class of
    perturbation -- so this shows that the tolerances and caps are reachable by the reference alone, with K = 8 from counting
    roundings and nothing fitted to the kernel.
  * THE EMULATION AGAINST THE MODEL.  sphere_t emulated in float32 (fast_model.emulate_sphere_t) with the root selection
    before the zero-root fix and the shipped one: on the zero-root scene the first must fail the model, the second pass it.
    That pins the model's rule for an origin exactly on a sphere without a GPU."""
import numpy as np
import pytest

import fast_model as fm


@pytest.fixture(scope="module")
def all_cases(pt):
    return fm.cases(pt)


CASE_NAMES = fm.case_names()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_oracle_passes_every_check_of_every_case(pt, oracle, all_cases, name):
    case = all_cases[name]
    frame = oracle.render(case.width, case.height, 1, spheres=case.spheres, basis=case.basis, eye=case.eye, max_bounces=case.max_bounces)
    v = case.check(frame, ib=0)  # the reference ranks with plain compares
    print(f"{name}: undecided {100 * v.stats['undecided']:.2f} % (cap {case.cap}), worst |t - t_model| / tol {v.stats['worst_t_ratio']:.3f}, "
          f"worst normal ratio {v.stats['worst_normal_ratio']:.3f}")
    assert v, str(v)
    if case.family == "on_surface_outward":  # the sphere under the eye is never returned at t = 0
        assert (v.t[v.idx >= 0] > 0).all()
    if case.family == "zero_root":
        assert (v.idx >= 0).all()  # nothing escapes: every ray meets the far side of the sphere it starts on, or something nearer


def test_model_rules_for_an_origin_on_the_sphere():
    """c == 0 exactly: inward (h < 0) is a sure hit at -2h/a, outward or tangent (h >= 0) a maybe; a sphere around the origin
    is a sure hit at its far root; one behind the ray a sure miss."""
    g = np.array([[0, 0, 0], [0, 0, 0], [40, 0, 0]], dtype=np.float32)
    r2 = np.array([256, 16, 16], dtype=np.float32)
    o = np.array([[16, 0, 0]] * 3, dtype=np.float32)
    d = np.array([[-1, 0.25, 0], [1, 0.05, 0], [0, 1, 0]], dtype=np.float32)
    p = fm.Pairs(o, d, g, r2, ib=0)
    assert p.c[0, 0] == 0.0 and p.sure[0, 0] and p.t[0, 0] == 2 * 16 / (1 + 0.0625)
    assert p.sure[0, 1] and p.miss[0, 2]
    assert p.maybe[1, 0] and p.maybe[2, 0] and p.miss[1, 1] and p.sure[1, 2]
    m = fm.Rays(p)
    assert m.decided.tolist() == [True, False, False] and m.idx[0] == 1
    assert fm.index_bits(1) == 1 and fm.index_bits(2) == 1 and fm.index_bits(3) == 2 and fm.index_bits(9) == 4
    assert fm.index_bits(33) == 6 and fm.index_bits(64) == 6 and fm.index_bits(65) == 0


@pytest.mark.parametrize("keyed", [False, True], ids=["compares", "keys"])
def test_emulated_sphere_t_fails_the_zero_root_scene_before_the_fix_and_passes_with_it(pt, all_cases, keyed):
    case = all_cases["zero_root_generic_n2"]
    o, d = case.rays()
    g, radius, r2 = fm.geometry(case.spheres)
    ib = fm.index_bits(case.n) if keyed else 0
    model = case.model(ib)
    assert model.decided.all()
    aimed_at_b = model.idx == 1
    assert 0 < aimed_at_b.sum() < len(aimed_at_b) and ((model.idx == 0) | aimed_at_b).all()
    far = model.idx == 0
    assert np.allclose(model.t[far], (-2.0 * model.pairs.h[:, 0] / model.pairs.a[:, 0])[far], rtol=1e-15)

    idx, t = fm.emulate_nearest(o, d, g, r2, fixed=False, keyed=keyed)
    before = fm.check_hits(model, idx, t)
    print(f"before the fix ({'keys' if keyed else 'compares'}): {(idx < 0).sum()} of {len(idx)} rays escape, "
          f"{(idx[far] != 0).sum()} of {far.sum()} lose the far side; {before}")
    assert not before
    if keyed:  # the key (0 & ~imask) | 0 is below every valid key: sphere A wins every ranking and its t = 0 is then rejected
        assert (idx < 0).all()
    else:      # one compare per sphere: only the rays that should see A's far side lose it
        assert (idx[aimed_at_b] == 1).all() and (idx[far] < 0).all()

    idx, t = fm.emulate_nearest(o, d, g, r2, fixed=True, keyed=keyed)
    after = fm.check_hits(model, idx, t)
    print(f"with the fix: worst |t - t_model| / tol {after.stats['worst_t_ratio']:.3f}")
    assert after, str(after)
    assert (idx == model.idx).all()


def test_emulation_stays_inside_the_tolerance_on_cornell_rays(pt, all_cases):
    """The emulation itself against the model on the primary rays of the reference's scene: every decided ray strong, every
    ray weak, with both rankings (worst |t - t_model| / tol about 0.14 at K = 8: the float32 arithmetic uses a sixth of the room)."""
    case = all_cases["cornell_64x64_b5"]
    o, d = case.rays()
    g, radius, r2 = fm.geometry(case.spheres)
    for keyed in (False, True):
        model = case.model(fm.index_bits(case.n) if keyed else 0)
        idx, t = fm.emulate_nearest(o, d, g, r2, fixed=True, keyed=keyed)
        v = fm.check_hits(model, idx, t)
        print(f"cornell, {'keys' if keyed else 'compares'}: undecided {100 * v.stats['undecided']:.2f} %, worst ratio {v.stats['worst_t_ratio']:.3f}")
        assert v, str(v)
        assert v.stats["undecided"] <= case.cap


@pytest.mark.parametrize("name,keyed", [("cornell_64x64_b5", True), ("random_n65_closed", False)])
def test_emulation_on_secondary_rays_stays_under_the_cap(pt, all_cases, name, keyed):
    """Rays of the shape tests/test_fast_nearest_gpu.py feeds the kernel's nearest<> (origins 0.05 off a surface, unit
    directions), through the emulation: the checks and the 2 % cap on undecided rays are reachable in float32."""
    case = all_cases[name]
    o, d = fm.secondary_rays(case, 8192 + 37, seed=5)
    g, _, r2 = fm.geometry(case.spheres)
    idx, t = fm.emulate_nearest(o, d, g, r2, fixed=True, keyed=keyed)
    v = fm.check_ray_list(o, d, case.spheres, fm.index_bits(case.n) if keyed else 0, idx, t)
    print(f"{name}: undecided {100 * v.stats['undecided']:.2f} %, worst |t - t_model| / tol {v.stats['worst_t_ratio']:.3f}")
    assert v, str(v)
    assert v.stats["undecided"] <= 0.02


def test_the_nearest_hook_is_lab_only_and_validates_its_arguments(pt, lab):
    assert "pt_debug_fast_nearest" in lab.LAB_ABI and hasattr(lab.lib, "pt_debug_fast_nearest")
    assert not hasattr(pt.lib, "pt_debug_fast_nearest")
    fn = lab.lib.pt_debug_fast_nearest
    assert fn(None, 9, None, 0, 0, 0, 0, None, None) == -1            # no scene
    assert fn(1, 8, None, 0, 1, 0, 0x1FF, None, None) == -1           # the specialised build is the 9-sphere one
    assert fn(1, 9, None, 5, 0, 0, 0x1FF, None, None) == -1           # rays without buffers
    assert fn(1, 9, None, 0, 1, 1, 0x1FF, None, None) == 0            # no rays: nothing to do, no device touched
