"""The fast mode (csrc/pt_fast.hip) ray by ray: product library, 1 spp, every pixel one ray.

At 1 spp nothing is jittered: pixel (row, col) is the ray o = eye, d = lerp(lerp(B0, B1, col / w), lerp(B2, B3, col / w),
1 - row / h), and eye and the four corner directions are free.  Every sphere gets a colour and an emission of its own
(fast_model.unique_materials), so the frame states the first hit exactly: channels 6-8 the hit sphere's colour bits, 0-2
clamp(emission), 9 t itself, 3-5 the normal, 10-13 zero, a miss all zeros.  Each frame is held to the float64 model of
tests/fast_model.py (the tolerances are formulas written there; tests/test_fast_model_host.py holds the reference's CPU
restatement to the same checks and caps):

  STRONG on decided rays -- hit or miss and the sphere equal the model's, |t - t_model| <= tol, the normal within its bound of
         the model's normal at the kernel's own t, colour and albedo bits exact;
  WEAK   on all rays -- the sphere is one of the model's possible winners (or a miss where one is possible), t within tol of that
         sphere's model root, everything finite;
  the undecided share stays under the case's cap.

The cases (fast_model.cases) reach what the statistical acceptance of tests/test_fast_mode_gpu.py never runs: the generic keyed
ranking (n <= 64 with a run-time count), every index width 1 .. 6 of the key, the switch at 64 / 65 spheres from LDS and keys to
in-place reads and compares, eyes exactly on a sphere looking inward (the zero root: before the fix of sphere_t these frames
came back black), outward and along the tangent, grazing fans, shifted and scaled scenes, long directions, the planar layout
and a ragged row tile.  PT_FAST_RAYS_OUT=<file>: the worst ratios and undecided shares per case family as JSON
(profiles/fast_rays/rays.json)."""
import numpy as np
import pytest

import fast_model as fm

pytestmark = pytest.mark.gpu

CASE_NAMES = fm.case_names()


@pytest.fixture(scope="module")
def all_cases(pt):
    return fm.cases(pt)


def _render(pt, case, **kw):
    img, _ = pt.render_frame(case.width, case.height, 1, spheres=case.spheres, basis=case.basis, eye=case.eye, fast_math=True,
                             max_bounces=case.max_bounces, **kw)
    return img


def _hold(case, frame, tag=""):
    v = case.check(frame, ib=fm.index_bits(case.n))
    print(f"{case.name}{tag}: undecided {100 * v.stats['undecided']:.2f} % (cap {case.cap}), worst |t - t_model| / tol "
          f"{v.stats['worst_t_ratio']:.3f}, worst normal ratio {v.stats['worst_normal_ratio']:.3f}, {(v.idx < 0).sum()} of {len(v.idx)} rays miss")
    fm.record("frames:" + case.family, v.stats)
    assert v, str(v)
    return v


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_ray_of_the_frame_against_the_model(pt, gpu, all_cases, name):
    case = all_cases[name]
    r = pt.Renderer(case.width, case.height, 1, fast_math=True, max_bounces=case.max_bounces)
    assert r.kernel_info(case.n)["variant"] == pt.VARIANT_FAST
    r.destroy()
    frames = [_render(pt, case)]
    v = _hold(case, frames[0])
    if case.family == "cornell":  # the other generator is another instantiation of the kernel; 1 spp draws no jitter
        frames.append(_render(pt, case, rng_mode=pt.RNG_PHILOX))
        _hold(case, frames[1], " philox")
        if case.max_bounces == 1:  # ... and with one bounce nothing is drawn at all
            assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    if case.family == "zero_root":
        # an origin exactly on a sphere, heading inward: the far side of that sphere, or whatever lies in front of it
        assert (v.idx >= 0).all(), f"{(v.idx < 0).sum()} of {len(v.idx)} rays left a closed scene"
        m = case.model(fm.index_bits(case.n))
        if case.name.startswith("zero_root_generic"):
            assert m.decided.all() and set(np.unique(v.idx)) == {0, 1}
            far = v.idx == 0
            p = m.pairs
            assert np.all(np.abs(v.t[far] - (-2.0 * p.h[:, 0] / p.a[:, 0])[far]) <= m.tol[far])
    if case.family == "on_surface_outward":
        # the sphere under the eye is a MAYBE of every ray, so no ray is decided: what must hold is asserted on its own
        hit = v.idx >= 0
        assert (v.t[hit] > 0).all(), "a sphere returned at t = 0"
        assert hit.any(), "the spheres behind the one under the eye are seen"
        assert np.isfinite(frames[0]).all()


@pytest.mark.parametrize("name", ["cornell_41x67_b5", "cornell_41x67_b8"], ids=["specialised", "generic"])
def test_planar_layout_and_ragged_row_tile_carry_the_full_frames_bits(pt, gpu, all_cases, name):
    case = all_cases[name]
    full = _render(pt, case)
    _hold(case, full)
    bits = full.view(np.uint32)
    w, h = case.width, case.height
    planar = _render(pt, case, layout=pt.LAYOUT_PLANAR).reshape(-1)[:14 * w * h].reshape(14, h * w)
    assert np.array_equal(planar.T.view(np.uint32).reshape(h, w, 14), bits)
    b, e = 13, 41
    tile = _render(pt, case, row_begin=b, row_end=e)
    assert tile.shape == (e - b, w, 14) and np.array_equal(tile.view(np.uint32), bits[b:e])
    ptile = _render(pt, case, row_begin=b, row_end=e, layout=pt.LAYOUT_PLANAR).reshape(-1)[:14 * w * (e - b)].reshape(14, (e - b) * w)
    assert np.array_equal(ptile.T.view(np.uint32).reshape(e - b, w, 14), bits[b:e])
