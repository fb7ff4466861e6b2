"""Sky and sun without a device: the model (tests/sky_model.py, the definition of EXACTNESS.md A.24 in NumPy float32) against the
models it extends where they must agree bit for bit, against closed forms that do not come from it, and against its own frame
without sun sampling (same expectation; two wrong models must fail that check); the library's host surface; the command line."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lights_cases as LC
import lights_model as LM
import materials_cases as MC
import materials_model as MM
import sky_cases as SC
import sky_model as SM
from test_lights_host import SPP_EXPECT, _frame_mean_and_se

f32, f64 = np.float32, np.float64


def _same_stream(a, b):
    return np.array_equal(a.d, b.d) and all(np.array_equal(x, y) for x, y in zip(a.v, b.v))


# ---- 1. anchors, bit for bit, model against model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_closed_box_under_any_sky_is_the_frame_without_one(oracle, rng):
    """No ray leaves the reference's box: all 14 channels of lights_model / materials_model, with and without sampling."""
    box, basis, sincos = oracle.scene_cornell(), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    kw = dict(rng=rng, philox=oracle.philox, seed=7)
    for sky in (SC.SUNS["small"], SC.SUNLESS):
        got, info = SM.render_frame(12, 12, 2, box, basis, sincos, sky, MC.smallpt(), **kw)
        want, _ = MM.render_frame(12, 12, 2, box, basis, sincos, MC.smallpt(), **kw)
        assert info["escaped_primary"] == info["escaped_later"] == 0
        SC.assert_same_bits(got, want, f"closed box, materials model, {rng}")
    got, info = SM.render_frame(12, 12, 2, box, basis, sincos, SC.SUNLESS, MC.smallpt(), light_sampling=True, **kw)
    want, winfo = LM.render_frame(12, 12, 2, box, basis, sincos, MC.smallpt(), **kw)
    assert info["escaped_primary"] == info["escaped_later"] == 0 and LC.counters(info) == LC.counters(winfo)
    SC.assert_same_bits(got, want, f"closed box, lights model, {rng}")


@pytest.mark.parametrize("light_sampling", [False, True])
def test_black_sunless_sky_differs_from_no_sky_in_the_colour_variance_alone(oracle, light_sampling):
    sph, basis, sincos = SC.courtyard(oracle.scene_cornell()), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    got, info = SM.render_frame(12, 12, 4, sph, basis, sincos, SC.BLACK, SC.COURTYARD_SMALLPT, light_sampling=light_sampling, seed=3)
    want, _ = SM.render_frame(12, 12, 4, sph, basis, sincos, None, SC.COURTYARD_SMALLPT, light_sampling=light_sampling, seed=3)
    ref, _ = LM.render_frame(12, 12, 4, sph, basis, sincos, SC.COURTYARD_SMALLPT, light_sampling=light_sampling, seed=3)
    SC.assert_same_bits(want, ref, "sky=None is the lights model")
    assert info["escaped_primary"] >= 20 and info["escaped_later"] >= 20
    others = [c for c in range(14) if c != 10]
    SC.assert_same_bits(got[..., others], want[..., others], "black sky, channels 0-9 and 11-13")
    # channel 10 is the decision of A.24: every sample counts, so pixels whose samples all escaped have a count where they had none
    assert not got[..., :3].any() and not got[..., 10].any()  # an unlit scene: zero colour, zero variance either way


def test_lights_with_a_sunless_sky_take_the_draws_of_lights_alone(oracle):
    """The persisted XORWOW words after a frame: a sunless sky adds no light to A.23's list; a sun adds two draws per sampling bounce."""
    sph, basis, sincos = SC.courtyard_three_lamps(oracle.scene_cornell()), oracle.camera_basis(w=12, h=12), MM.sincos_of(oracle)
    _, alone = LM.render_frame(12, 12, 2, sph, basis, sincos, seed=5)
    _, sunless = SM.render_frame(12, 12, 2, sph, basis, sincos, SC.SUNLESS, light_sampling=True, seed=5)
    _, sunny = SM.render_frame(12, 12, 2, sph, basis, sincos, SC.SUNS["small"], light_sampling=True, seed=5)
    assert sunless["sampled"] >= 20 and sunless["sampled"] == alone["sampled"]
    assert _same_stream(sunless["state"], alone["state"])
    assert not _same_stream(sunny["state"], alone["state"])


# ---- 2. closed forms that do not come from the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw,pitch", SC.ESCAPE_VIEWS)
def test_every_primary_ray_escapes_is_the_sky_itself(oracle, yaw, pitch):
    """(a) 1 spp, one small sphere behind the camera: each pixel is clamp(rad(normalize(d)), 0, 1) from the basis alone, bit for bit."""
    size, sky = 24, SC.SUNS["in view"]
    basis = oracle.camera_basis(SC.EYE, yaw, pitch, w=size, h=size)
    img, info = SM.render_frame(size, size, 1, SC.behind_the_camera(), basis, MM.sincos_of(oracle), sky, light_sampling=True)
    assert info["escaped_primary"] == size * size
    n_up, n_down, n_sun = SC.assert_escape_frame(img, basis, size, sky, f"view {yaw} {pitch}")
    print(f"view {yaw} {pitch}: {n_up} pixels above the horizon, {n_down} below, {n_sun} inside the sun's cone")
    assert (n_up, n_down, n_sun) == (info["up"], info["ground"], info["sun_kept"])


def test_the_escape_views_cover_horizon_ground_and_the_suns_edge(oracle):
    seen = [SC.escape_closed_form(oracle.camera_basis(SC.EYE, yaw, pitch, w=24, h=24), 24, SC.SUNS["in view"])[1:] for yaw, pitch in SC.ESCAPE_VIEWS]
    assert any(up >= 20 and down >= 20 for up, down, _ in seen)          # the horizon line crosses a frame
    assert any(20 <= sun <= 24 * 24 - 20 for _, _, sun in seen)          # the sun's edge crosses a frame
    assert any(down > up for up, down, _ in seen)                        # a frame that is mostly ground


@pytest.mark.parametrize("light_sampling", [False, True])
def test_furnace_ball_under_a_uniform_sky_is_a_quarter(oracle, light_sampling):
    """(b) a uniform sky of 0.5, one DIFFUSE ball of colour 0.5, 4 spp, 3 bounces: colour exactly 0.25, colour variance exactly 0."""
    basis = oracle.camera_basis(w=24, h=24)
    img, info = SM.render_frame(24, 24, 4, SC.furnace_ball(), basis, MM.sincos_of(oracle), SC.FURNACE_SKY, max_bounces=3, light_sampling=light_sampling)
    whole = SC.assert_furnace_frame(img, "furnace (model)")
    print(f"furnace: {whole} pixels wholly on the ball; {SC.counters(info)}")
    assert info["capped"] == 0  # convex: every bounce leaves


def test_sun_on_a_floor_is_the_closed_form(oracle):
    """(c) tests/sky_cases.py: sun_floor_closed_form and SUN_FLOOR_ROUNDINGS say what is held and why."""
    size = 24
    basis = oracle.camera_basis(SC.SUN_FLOOR_EYE, SC.SUN_FLOOR_YAW, SC.SUN_FLOOR_PITCH, w=size, h=size)
    kw = dict(eye=SC.SUN_FLOOR_EYE, max_bounces=2)
    img, info = SM.render_frame(size, size, 1, SC.floor_only(), basis, MM.sincos_of(oracle), SC.SUN_FLOOR_SKY, light_sampling=True, **kw)
    off, _ = SM.render_frame(size, size, 1, SC.floor_only(), basis, MM.sincos_of(oracle), SC.SUN_FLOOR_SKY, light_sampling=False, **kw)
    covered, passed, widest = SC.sun_floor_closed_form(img, basis, size)
    _, passed_off, _ = SC.sun_floor_closed_form(off, basis, size)
    print(f"sun on a floor: {covered} floor pixels, {passed} inside the interval (sampling off: {passed_off}); widest interval {widest:.5f} of the scale; "
          f"{SC.counters(info)}")
    assert covered >= 500 and widest < 0.01
    assert passed == covered
    assert passed_off < 0.05 * covered  # a cosine bounce finds a cone of 0.006 sr twice in a thousand tries


# ---- 3. same expectation ------------------------------------------------------------------------------------------------------------------
def test_frame_mean_is_the_same_with_and_without_sun_sampling(oracle):
    """Sampling the sun changes the noise, not the picture: the 8 x 8 courtyard under the wide sun, 3 bounces, fixed seeds,
    lights_model's own SPP_EXPECT and 4-standard-error bound (under a sky every sample enters channel 10, so the bound's standard
    error holds for an open scene).  The same check must FAIL for a model that ignores the flag (the sun counted twice) and for one
    that drops the sun from every later escape (the light of unsampled paths lost)."""
    sph, basis, sincos = SC.courtyard(oracle.scene_cornell()), oracle.camera_basis(w=8, h=8), MM.sincos_of(oracle)
    sky, frames = SC.SUNS["wide"], {}
    for name, kw in (("on", dict(seed=11, light_sampling=True)), ("off", dict(seed=12)), ("double", dict(seed=11, light_sampling=True, wrong="double")),
                     ("drop", dict(seed=12, wrong="drop"))):
        img, info = SM.render_frame(8, 8, SPP_EXPECT, sph, basis, sincos, sky, max_bounces=3, **kw)
        frames[name] = _frame_mean_and_se(img, SPP_EXPECT) + (info,)
    (m_on, se_on, i_on), (m_off, se_off, i_off) = frames["on"], frames["off"]
    bound = 4.0 * np.hypot(se_on, se_off)
    print(f"same expectation: mean on {m_on:.5f} (se {se_on:.5f}) off {m_off:.5f} (se {se_off:.5f}): |difference| {abs(m_on - m_off):.5f} <= bound {bound:.5f}; "
          f"{SC.counters(i_on)}")
    assert i_on["sun_suppressed"] >= 20 and i_on["sun_lit"] >= 20 and i_off["sun_kept"] >= 20
    assert abs(m_on - m_off) <= bound
    for wrong, against in (("double", "off"), ("drop", "on")):
        m_w, se_w, _ = frames[wrong]
        m_r, se_r, _ = frames[against]
        bound_w = 4.0 * np.hypot(se_w, se_r)
        print(f"  wrong model '{wrong}': mean {m_w:.5f} against {against} {m_r:.5f}: |difference| {abs(m_w - m_r):.5f} > its bound {bound_w:.5f} "
              f"(margin {abs(m_w - m_r) / bound_w:.2f} x)")
        assert abs(m_w - m_r) > bound_w


# ---- 4. pt_sky_check ------------------------------------------------------------------------------------------------------------------------
GOOD = dict(zenith=(0.2, 0.4, 0.8), horizon=(0.8, 0.85, 0.9), ground=(0.25, 0.25, 0.25), sun_dir=(0.4, 0.8, 0.45), sun_cos=0.999, sun_radiance=(4.0, 3.0, 2.0))
REFUSALS = [
    (dict(zenith=(0.2, float("nan"), 0.8)), r"pt_sky_check: zenith\[1\] is not finite"),
    (dict(horizon=(float("inf"), 0.85, 0.9)), r"pt_sky_check: horizon\[0\] is not finite"),
    (dict(ground=(0.25, 0.25, -0.5)), r"pt_sky_check: ground\[2\] -0.5 is negative"),
    (dict(sun_radiance=(4.0, -1.0, 2.0)), r"pt_sky_check: sun_radiance\[1\] -1 is negative"),
    (dict(sun_radiance=(4.0, float("inf"), 2.0)), r"pt_sky_check: sun_radiance\[1\] is not finite"),
    (dict(sun_dir=(0.4, float("nan"), 0.45)), r"pt_sky_check: sun_dir\[1\] is not finite"),
    (dict(sun_dir=(0.0, 0.0, 0.0)), r"pt_sky_check: sun_dir \(0, 0, 0\) has no direction"),
    (dict(sun_dir=(0.0, 1e30, 0.0)), r"pt_sky_check: sun_dir \(0, 1e\+30, 0\) has no direction"),  # its squared length is inf in float32
    (dict(sun_cos=1.0), r"pt_sky_check: sun_cos 1 \(the cosine of the sun's angular radius: 0 <= sun_cos < 1\)"),
    (dict(sun_cos=-0.25), r"pt_sky_check: sun_cos -0.25 \("),
    (dict(sun_cos=float("nan")), r"pt_sky_check: sun_cos nan \("),
    (dict(sun_cos=1.0 - 2.0 ** -21), r"pt_sky_check: sun_cos 0.99999952\d* is too near 1 \(1 - sun_cos must be at least 2\^-20\)"),
]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_sky_check_refuses_by_name(pt, change, message):
    with pytest.raises(pt.PtError, match=message) as e:
        pt.sky_check(pt.Sky(**dict(GOOD, **change)))
    assert e.value.code == -1  # PT_EINVAL


def test_sky_check_takes_what_is_good(pt):
    pt.sky_check(pt.Sky(**GOOD))
    pt.sky_check(pt.CLEAR_SKY)
    pt.sky_check(pt.Sky(**dict(GOOD, sun_cos=1.0 - 2.0 ** -20)))  # the bound itself
    pt.sky_check(pt.Sky(**dict(GOOD, sun_cos=0.0)))               # a hemisphere
    # without a sun its direction and cosine are not read
    pt.sky_check(pt.Sky(GOOD["zenith"], GOOD["horizon"], GOOD["ground"]))
    pt.sky_check(pt.Sky(**dict(GOOD, sun_radiance=(0.0, 0.0, 0.0), sun_dir=(0.0, 0.0, 0.0), sun_cos=7.0)))
    with pytest.raises(pt.PtError, match=r"pt_sky_check: sky is NULL"):
        pt.sky_check(None)
    assert pt.lib.pt_renderer_set_sky(None, None) == -1 and b"pt_renderer_set_sky: renderer is NULL" in pt.lib.pt_last_error()


# ---- 5, 6. surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_libraries_export(pt, lab):
    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pt_sky_check\s*\(\s*const\s+pt_sky\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+pt_renderer_set_sky\s*\(\s*pt_renderer\s*\*\s*\w+\s*,\s*const\s+pt_sky\s*\*\s*\w+\s*\)", code)
    for name in ("pt_sky_check", "pt_renderer_set_sky"):
        assert name in pt.ABI and hasattr(ctypes.CDLL(pt.LIB_PATH), name) and hasattr(ctypes.CDLL(lab.LIB_PATH), name)
    assert "src/pathtrace.cu:157-161" in text[text.index("sky and sun"):text.index("pt_sky_check")]  # cites what it departs from
    assert int(re.search(r"#define PT_VARIANT_MATERIALS_SKY (\d+)", code).group(1)) == pt.VARIANT_MATERIALS_SKY == 103
    assert int(re.search(r"#define PT_VARIANT_MATERIALS_LIGHTS_SKY (\d+)", code).group(1)) == pt.VARIANT_MATERIALS_LIGHTS_SKY == 104
    fields = re.search(r"typedef struct pt_sky \{(.*?)\} pt_sky;", code, flags=re.S).group(1)
    assert re.findall(r"float\s+(\w+)(?:\[3\])?;", fields) == [n for n, _ in pt.PtSky._fields_] and ctypes.sizeof(pt.PtSky) == 16 * 4
    host = os.path.join(ROOT, "cuda-pathtrace_amd", "host")
    assert "SetSky(const pt_sky*" in open(os.path.join(host, "Renderer.h")).read() and os.path.exists(os.path.join(host, "Sky.h"))
    assert not hasattr(pt.MultiRenderer, "set_sky")


def test_the_abi_is_additive(pt):
    assert pt.lib.pt_abi_version() == 6 and ctypes.sizeof(pt.RendererOpts) == 48


def test_clear_sky_is_what_the_documents_say(pt):
    from conftest import ROOT

    c = pt.CLEAR_SKY
    assert max(c.sun_radiance) / max(c.zenith + c.horizon) >= 100 and 0.99 < c.sun_cos < 1 and c.as_dict() == SC.SUNS["small"]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Sky and sun (`--sky`)" in readme
    section = readme[readme.index("## Sky and sun (`--sky`)"):]
    for figure in ("(0.18, 0.36, 0.80)", "(0.80, 0.85, 0.90)", "(0.4, 0.8, 0.45)", "0.999", "(400, 380, 340)"):
        assert figure in section, figure


# ---- 7. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    from conftest import ROOT

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    return subprocess.run([exe, "--size", "16", "-s", "1", "--nobitmap", "--device", "99"] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,other", [(["--progressive", "2"], "--progressive"), (["--poses", "x", "--batch"], "--batch"), (["--gpus", "2"], "--gpus")])
def test_cli_refuses_combinations_before_a_device(extra, other):
    res = _cli("--sky", "clear", *extra)
    assert res.returncode == 1 and f"--sky cannot be combined with {other}" in res.stderr and "GPUassert" not in res.stderr, res.stderr


BAD_FILES = [
    ("zenith 1 1 1\nsunny 1 2 3\n", "line 2: key 'sunny' is none of zenith, horizon, ground, sun"),
    ("zenith 1 1\n", "line 1: expected 'zenith r g b'"),
    ("zenith 1 1 1 1\n", "line 1: expected 'zenith r g b'"),
    ("ground 1 x 1\n", "line 1: expected 'ground r g b'"),
    ("# only the direction\nsun 0 1 0\n", "line 2: expected 'sun dx dy dz cos r g b'"),
    ("horizon 1 1 1\nhorizon 1 1 1\n", "line 2: 'horizon' is repeated"),
    ("# nothing\n\n", "no sky in "),
    ("zenith 1 nan 1\n", "pt_sky_check: zenith[1] is not finite"),
    ("sun 0 0 0 0.99 5 5 5\n", "pt_sky_check: sun_dir (0, 0, 0) has no direction"),
    ("sun 0 1 0 1.5 5 5 5\n", "pt_sky_check: sun_cos 1.5 ("),
]


@pytest.mark.parametrize("text,message", BAD_FILES)
def test_cli_sky_file_parser_refuses_by_line(tmp_path, text, message):
    path = tmp_path / "sky.txt"
    path.write_text(text)
    res = _cli("--sky", str(path))
    assert res.returncode == 1 and "ERROR: --sky: " in res.stderr and message in res.stderr and "GPUassert" not in res.stderr, res.stderr


def test_cli_takes_a_good_sky(tmp_path):
    """A good command line passes every host check: the run then stops at the device it was told to use (--device 99), not before."""
    path = tmp_path / "sky.txt"
    path.write_text("# a sky\nzenith 0.1 0.2 0.3\n\nsun 0 1 0 0.99 5 5 5\n")  # unlisted lines are zero
    missing = _cli("--sky", str(tmp_path / "none.txt"))
    assert missing.returncode == 1 and "cannot open sky file" in missing.stderr
    for args in (["--sky", "clear"], ["--sky", str(path), "--direct-light"], ["--materials", "smallpt", "--sky", "clear", "--direct-light", "--frames", "2"],
                 ["--sky", "clear", "--temporal", "--filter", "--tonemap", "aces", "--frames", "2"]):
        res = _cli(*args)
        assert res.returncode != 0 and "GPUassert:" in res.stderr and "--sky" not in res.stderr, (args, res.stderr)
    from conftest import ROOT

    usage = subprocess.run([os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--sky" in usage.stdout + usage.stderr
