"""Direct light sampling without a device: the model (tests/lights_model.py, the definition of EXACTNESS.md A.23 in NumPy float32)
against the materials model where the two must agree bit for bit, against a closed form, and against its own frame without the
option (same expectation, lower variance); the library's host surface; the command line's refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import lights_cases as LC
import lights_model as LM
import materials_cases as MC
import materials_model as MM

f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32


def _lum(img):
    return 0.2126 * img[..., 0].astype(f64) + 0.7152 * img[..., 1].astype(f64) + 0.0722 * img[..., 2].astype(f64)


# ---- 1. anchors, bit for bit ------------------------------------------------------------------------------------------------------------
def test_no_light_and_one_bounce_are_the_materials_frame(oracle):
    box, basis, sincos = oracle.scene_cornell(), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    for what, sph, mb in (("no light", LC.no_light_box(box), 5), ("max_bounces 1", LC.small_lamp_box(box), 1)):
        for rng in ("xorwow", "philox"):
            kw = dict(max_bounces=mb, rng=rng, philox=oracle.philox, seed=7)
            got, info = LM.render_frame(12, 12, 2, sph, basis, sincos, MC.smallpt(), **kw)
            want, winfo = MM.render_frame(12, 12, 2, sph, basis, sincos, MC.smallpt(), **kw)
            LC.assert_same_bits(got, want, f"{what} {rng}")
            assert info["sampled"] == info["suppressed"] == 0 and MC.arms(info) == MC.arms(winfo)
            if rng == "xorwow":  # the stream did not move either
                assert np.array_equal(info["state"].d, winfo["state"].d) and all(np.array_equal(a, b) for a, b in zip(info["state"].v, winfo["state"].v))


def test_furnace_under_philox_is_the_materials_frame(oracle):
    """Every diffuse point of the furnace lies inside its one light (the wall, radius 300), and the wall's own hits are `self`: no
    sample is ever formed, nothing is marked, and Philox's path draws do not move.  (Under XORWOW the light draws move the stream.)"""
    sph, basis, sincos = MC.ball_furnace(), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    table = [(MC.DIFFUSE, 0.0), (MC.DIFFUSE, 0.0)]
    kw = dict(max_bounces=4, rng="philox", philox=oracle.philox, seed=0x300000005, frame=1)
    got, info = LM.render_frame(12, 12, 2, sph, basis, sincos, table, **kw)
    want, _ = MM.render_frame(12, 12, 2, sph, basis, sincos, table, **kw)
    print("furnace:", LC.counters(info))
    assert info["inside"] >= 20 and info["self"] >= 20 and info["sampled"] == 0 and info["suppressed"] == 0 and info["kept"] >= 20
    LC.assert_same_bits(got, want, "furnace, philox")
    _, moved = LM.render_frame(12, 12, 2, sph, basis, sincos, table, max_bounces=4)
    _, still = MM.render_frame(12, 12, 2, sph, basis, sincos, table, max_bounces=4)
    assert not np.array_equal(moved["state"].d, still["state"].d)  # XORWOW: two more draws per sampling bounce


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_option_off_is_the_materials_frame(oracle, rng):
    box, basis, sincos = oracle.scene_cornell(), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    for sph, table in ((LC.small_lamp_box(box), MC.smallpt()), (LC.three_lamp_box(box), [(MC.DIFFUSE, 0.0)] * 11), (box, None)):
        kw = dict(rng=rng, philox=oracle.philox, seed=3)
        got, info = LM.render_frame(12, 12, 2, sph, basis, sincos, table, light_sampling=False, **kw)
        want, _ = MM.render_frame(12, 12, 2, sph, basis, sincos, table if table is not None else [(MC.DIFFUSE, 0.0)] * len(sph), **kw)
        LC.assert_same_bits(got, want, f"option off, {len(sph)} spheres, {rng}")
        assert info["sampled"] == info["suppressed"] == info["kept"] == 0


# ---- 2. closed form ---------------------------------------------------------------------------------------------------------------------
def test_floor_under_a_small_lamp_is_the_closed_form(oracle):
    """Floor and lamp, 1 spp (no jitter), max_bounces = 2: a pixel whose first hit is the floor holds exactly one light sample --
    bounce 1 adds nothing: the floor does not emit and the lamp, if hit, has been accounted for -- so its colour is
    albedo * Le * 2 vers * cos(angle between nl and l), and l lies within a = asin(r / d) of the lamp's centre:
        colour in albedo * Le * 2 vers * [cos(theta + a), cos(max(theta - a, 0))],
    theta, a, d and vers = 1 - cos(a) in float64 from the pixel's ray (the basis) and its depth channel.  The interval is widened by
    LC.FLOOR_ROUNDINGS = 64 float32 roundings, relative and absolute (in units of albedo * Le * 2 vers): the model spends about 45 operations
    between the eye and the gain (hit point 2 per component, normal 5, origin 2, sw 1, d2 5, q, cmax, vers 5, h, cos_a, sin_a 5, the
    frame's three normalisations 15, l 10, cosl 5, the gain 4), each at most one unit roundoff of a quantity no larger than the
    scale, and the float64 side reads a hit point that the depth channel's own rounding moved by at most one more.
    The camera looks down at the floor under the lamp (theta < 3 degrees) and r / d = 0.1, so theta + a < 0.141 and the interval,
    1 - cos(theta + a) of the scale, is narrower than 1 % (asserted); tests/lights_cases.py says why r / d is not smaller."""
    size = 24
    sph, sincos = LC.floor_and_lamp(), MM.sincos_of(oracle)
    basis = oracle.camera_basis(LC.FLOOR_EYE, LC.FLOOR_YAW, LC.FLOOR_PITCH, w=size, h=size)
    img, info = LM.render_frame(size, size, 1, sph, basis, sincos, eye=LC.FLOOR_EYE, max_bounces=2)
    off, _ = LM.render_frame(size, size, 1, sph, basis, sincos, eye=LC.FLOOR_EYE, max_bounces=2, light_sampling=False)
    covered, passed, widest = LC.floor_closed_form(img, basis, size)
    _, passed_off, _ = LC.floor_closed_form(off, basis, size)
    print(f"closed form: {covered} floor pixels, {passed} inside the interval (option off: {passed_off}); widest interval {widest:.5f} of the scale; "
          f"{LC.counters(info)}")
    assert covered >= 200 and widest < 0.01
    assert passed == covered
    assert passed_off < 0.05 * covered  # without the feature a bounce essentially never finds the lamp


# ---- 3. same expectation ----------------------------------------------------------------------------------------------------------------
SPP_EXPECT = 384


def _frame_mean_and_se(img, spp):
    """Mean luminance of the frame and its standard error: channel 10 is each pixel's variance over ALL its samples (every path of a
    closed scene scores), so the pixel mean's variance is channel 10 / spp and the frame mean's is their sum / pixels^2."""
    n = img.shape[0] * img.shape[1]
    return _lum(img).mean(), np.sqrt(img[..., 10].astype(f64).sum() / spp) / n


def test_frame_mean_is_the_same_with_and_without(oracle):
    """The option changes the noise, not the picture: 8 x 8, 3 bounces, a lamp of radius 8 in the closed box, fixed seeds.  The same
    check must FAIL for a model that ignores the mask of sampled lights (it counts direct light twice)."""
    sph, basis, sincos = LC.medium_lamp_box(oracle.scene_cornell()), oracle.camera_basis(w=8, h=8), MM.sincos_of(oracle)
    frames = {}
    for name, kw in (("on", dict(seed=11)), ("off", dict(seed=12, light_sampling=False)), ("mutant", dict(seed=11, double_count=True))):
        img, info = LM.render_frame(8, 8, SPP_EXPECT, sph, basis, sincos, max_bounces=3, **kw)
        assert info["capped"] == info["paths"]  # closed: every path scores
        frames[name] = _frame_mean_and_se(img, SPP_EXPECT) + (info,)
    (m_on, se_on, i_on), (m_off, se_off, _), (m_mut, se_mut, _) = frames["on"], frames["off"], frames["mutant"]
    bound, bound_mut = 4.0 * np.hypot(se_on, se_off), 4.0 * np.hypot(se_mut, se_off)
    print(f"same expectation: mean on {m_on:.5f} (se {se_on:.5f}) off {m_off:.5f} (se {se_off:.5f}): |difference| {abs(m_on - m_off):.5f} <= "
          f"bound {bound:.5f}; mutant mean {m_mut:.5f}: |difference| {abs(m_mut - m_off):.5f} against its bound {bound_mut:.5f} "
          f"(margin {abs(m_mut - m_off) / bound_mut:.2f} x); {LC.counters(i_on)}")
    assert i_on["suppressed"] >= 20 and i_on["lit"] >= 20
    assert abs(m_on - m_off) <= bound
    assert abs(m_mut - m_off) > bound_mut


def test_frame_mean_is_the_same_with_glossy_balls(oracle):
    """GLOSSY is treated as specular: it never samples, clears the set of sampled lights, and a lamp hit after it keeps its light.
    Were a GLOSSY hit to sample (it has no pdf to weight the sample by) or to leave the set standing, the mean would move: the same
    check, with the box's two balls GLOSSY 0.3 and 5 bounces (at 3 a lamp of radius 8 is hit after a glossy bounce 12 times)."""
    sph, basis, sincos = LC.medium_lamp_box(oracle.scene_cornell()), oracle.camera_basis(w=8, h=8), MM.sincos_of(oracle)
    on, info = LM.render_frame(8, 8, SPP_EXPECT, sph, basis, sincos, LC.GLOSSY_BALLS, max_bounces=5, seed=21)
    off, _ = LM.render_frame(8, 8, SPP_EXPECT, sph, basis, sincos, LC.GLOSSY_BALLS, max_bounces=5, seed=22, light_sampling=False)
    (m_on, se_on), (m_off, se_off) = _frame_mean_and_se(on, SPP_EXPECT), _frame_mean_and_se(off, SPP_EXPECT)
    bound = 4.0 * np.hypot(se_on, se_off)
    print(f"glossy balls: mean on {m_on:.5f} (se {se_on:.5f}) off {m_off:.5f} (se {se_off:.5f}): |difference| {abs(m_on - m_off):.5f} <= bound {bound:.5f}; "
          f"glossy hits {info['glossy']}, {LC.counters(info)}")
    assert info["glossy"] >= 20 and info["kept_after_glossy"] >= 20 and info["suppressed"] >= 20
    assert abs(m_on - m_off) <= bound


# ---- 4. variance ------------------------------------------------------------------------------------------------------------------------
def test_small_lamp_box_has_less_variance_with_the_option(oracle):
    sph, basis, sincos = LC.small_lamp_box(oracle.scene_cornell()), oracle.camera_basis(w=24, h=24), MM.sincos_of(oracle)
    on, _ = LM.render_frame(24, 24, 8, sph, basis, sincos, seed=5)
    off, _ = LM.render_frame(24, 24, 8, sph, basis, sincos, seed=5, light_sampling=False)
    v_on, v_off = on[..., 10].astype(f64).sum(), off[..., 10].astype(f64).sum()
    print(f"small-lamp box, 24 x 24 x 8 spp: colour variance summed over the frame, on {v_on:.4g} off {v_off:.4g}: ratio {v_on / v_off:.4g}; "
          f"pixels with any light: on {np.count_nonzero(_lum(on) > 0)} off {np.count_nonzero(_lum(off) > 0)} of 576")
    assert v_on < v_off


# ---- 5. surface -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_libraries_export(pt, lab):
    import ctypes

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "pt_renderer_set_light_sampling"
    assert re.search(r"\bint\s+%s\s*\(\s*pt_renderer\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)" % name, code)
    assert name in pt.ABI and hasattr(ctypes.CDLL(pt.LIB_PATH), name) and hasattr(ctypes.CDLL(lab.LIB_PATH), name)
    assert "src/pathtrace.cu" in text[text.index("direct light sampling"):text.index(name)]  # cites what it departs from
    assert int(re.search(r"#define PT_VARIANT_MATERIALS_LIGHTS (\d+)", code).group(1)) == pt.VARIANT_MATERIALS_LIGHTS == pt.VARIANT_MATERIALS + 1
    assert pt.lib.pt_abi_version() == 6 and ctypes.sizeof(pt.RendererOpts) == 48
    assert "SetLightSampling(bool" in open(os.path.join(ROOT, "cuda-pathtrace_amd", "host", "Renderer.h")).read()
    assert not hasattr(pt.MultiRenderer, "set_light_sampling")


def test_null_renderer_is_refused_by_name(pt):
    for on in (0, 1):
        assert pt.lib.pt_renderer_set_light_sampling(None, on) == -1  # PT_EINVAL
        assert b"pt_renderer_set_light_sampling: renderer is NULL" in pt.lib.pt_last_error()


def _cli(*args):
    from conftest import ROOT

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    return subprocess.run([exe, "--size", "16", "-s", "1", "--nobitmap", "--device", "99"] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("materials", [[], ["--materials", "smallpt"]])
@pytest.mark.parametrize("extra,other", [(["--progressive", "2"], "--progressive"), (["--poses", "x", "--batch"], "--batch"), (["--gpus", "2"], "--gpus")])
def test_cli_refuses_combinations_before_a_device(materials, extra, other):
    res = _cli("--direct-light", *materials, *extra)
    flag = "--materials" if materials else "--direct-light"  # the table's own refusal comes first
    assert res.returncode == 1 and f"{flag} cannot be combined with {other}" in res.stderr and "GPUassert" not in res.stderr, res.stderr


def test_cli_takes_the_flag_alone_and_with_a_table():
    """A good command line passes every host check: the run then stops at the device it was told to use (--device 99), not before."""
    for args in (["--direct-light"], ["--direct-light", "--materials", "smallpt"], ["--materials", "smallpt", "--direct-light", "--frames", "2"]):
        res = _cli(*args)
        assert res.returncode != 0 and "GPUassert:" in res.stderr and "--direct-light" not in res.stderr, res.stderr
    from conftest import ROOT

    usage = subprocess.run([os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--direct-light" in usage.stdout + usage.stderr
