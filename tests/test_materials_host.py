"""Sphere materials without a device: the model (tests/materials_model.py, the definition of EXACTNESS.md A.22 in NumPy float32)
against the restatement and the oracle, against closed forms and against float64; the library's host checks; the command line's
parsing and refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import materials_cases as MC
import materials_model as MM
import numpy_restatement as NR

f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32


# ---- 1. anchor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [4, 1])
def test_all_diffuse_model_is_the_restatement_and_the_oracle(oracle, spp):
    sph, basis, sincos = oracle.scene_cornell(), oracle.camera_basis(w=16, h=16), MM.sincos_of(oracle)
    table = [(MC.DIFFUSE, 0.0)] * 9
    got, info = MM.render_frame(16, 16, spp, sph, basis, sincos, table)
    MC.assert_same_bits(got, NR.render_frame(16, 16, spp, sph, basis, sincos), f"xorwow {spp} spp")
    assert info["diffuse"] == 16 * 16 * spp * 5 and info["capped"] == info["paths"] and sum(info[a] for a in MM.ARMS[1:]) == 0
    got, _ = MM.render_frame(16, 16, spp, sph, basis, sincos, table, rng="philox", philox=oracle.philox, seed=0x500000003, frame=2)
    MC.assert_same_bits(got, oracle.render(16, 16, spp, sph, basis, rng_mode=1, seed=0x500000003, frame=2), f"philox {spp} spp")


# ---- 2. closed form: the mirror furnace ----------------------------------------------------------------------------------------------
def test_mirror_furnace_is_exactly_the_emission(oracle):
    """On the mirror a pixel holds 0 + 1 * E at bounce 1 (the wall's colour 0 ends the path's weight), off it clamp(E) = E at bounce
    0; four equal dyadic values sum and divide exactly, and equal luminances leave the colour variance 0.  Written without the model's
    help: the expected frame is E."""
    sph, basis = MC.ball_furnace(), oracle.camera_basis(w=16, h=16)
    img, info = MM.render_frame(16, 16, 4, sph, basis, MM.sincos_of(oracle), [(MC.DIFFUSE, 0.0), (MC.MIRROR, 0.0)], max_bounces=3)
    assert info["mirror"] >= 20 and info["mirror"] < info["paths"]
    for k in range(3):
        assert np.all(img[..., k] == f32(MC.E[k])), k
    assert np.all(img[..., 10] == 0.0)


# ---- 3. one bounce against float64 ---------------------------------------------------------------------------------------------------
def _one_bounce(eta, inside):
    """A fan of incidence angles 0.5, 1, ... 89.5 degrees on a surface in general position, rays of length 1.7: the model's step and
    the same quantities in float64 from the very float32 inputs."""
    theta = np.deg2rad(np.arange(0.5, 90.0, 0.5))
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # orthonormal
    n_loc = np.array([0.0, 0.0, 1.0])
    d_loc = np.stack([np.sin(theta), np.zeros_like(theta), (1.0 if inside else -1.0) * np.cos(theta)], axis=1) * 1.7
    nr = NR._normalize([np.full(theta.shape, f32((rot @ n_loc)[k])) for k in range(3)])
    d = [(d_loc @ rot.T)[:, k].astype(f32) for k in range(3)]
    front = NR._dot(nr, d) < 0
    assert np.all(front != inside)
    nl = [np.where(front, nr[k], (f32(-1.0) * nr[k]).astype(f32)) for k in range(3)]
    inv, r0 = MM.glass_constants(eta)
    n = len(theta)
    c = [np.full(n, f32(v)) for v in (0.6, 0.0, 0.8)]
    full = lambda v, t=f32: np.full(n, v, dtype=t)  # noqa: E731
    _, d_next, decided, _, _, x = MM.material_step([full(0.0)] * 3, nl, nr, front, d, c, full(0.5), full(MC.GLASS, np.int32), full(eta), full(inv),
                                                   full(r0))
    # float64 from the float32 inputs
    eta64 = f64(f32(eta))
    n64 = np.stack([v.astype(f64) for v in nr], axis=1)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    d64 = np.stack([v.astype(f64) for v in d], axis=1)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    cos_i = np.abs(np.sum(n64 * d64, axis=1))
    sin_i = np.linalg.norm(np.cross(n64, d64), axis=1)
    nnt = eta64 if inside else 1.0 / eta64
    sin_t = nnt * sin_i
    td = np.stack([v.astype(f64) for v in x["td"]], axis=1)
    sin_t_model = np.linalg.norm(np.cross(n64, td), axis=1) / np.linalg.norm(td, axis=1)
    cos_t = np.sqrt(np.maximum(1.0 - sin_t * sin_t, 0.0))
    r0_64 = ((eta64 - 1.0) / (eta64 + 1.0)) ** 2
    schlick = r0_64 + (1.0 - r0_64) * (1.0 - (cos_t if inside else cos_i)) ** 5
    return dict(nnt=nnt, sin_t=sin_t, sin_t_model=sin_t_model, cos_t=cos_t, schlick=schlick, re=x["re"].astype(f64), tir=x["tir"], decided=decided,
                d_next=d_next, m=x["m"], td=x["td"])


@pytest.mark.parametrize("eta", [1.33, 1.5, 2.4])
@pytest.mark.parametrize("inside", [False, True])
def test_one_bounce_obeys_snell_and_schlick_in_float64(eta, inside):
    """Bounds from float32 rounding alone (u = 2^-24, a few ulps per operand; nnt = eta from inside, 1 / eta from outside):
      k = 1 - nnt^2 (1 - ddn^2) carries at most 20 u max(1, nnt^2): du and nl are each within 4 u, their dot within 7 u, the products
        and differences add the rest;
      Snell: the tangential part of td is du's times nnt (6 u), the normal part is -sqrt(k) plus a cancellation residue of at most
        20 u nnt, and |td|^2 = tangential^2 + k, so   |nnt sin(i) - sin(t)| <= (10 + 10 max(1, nnt^2) + 20 nnt) u;
      Schlick: Re moves by at most 5 |d cx| + 12 u (the fifth power's slope is at most 5, its four products and the blend with R0
        add the 12 u); from outside cx = -ddn, |d cx| <= 8 u; from inside cx = td . nr = sqrt(k) / |td|, whose error near the critical
        angle is k's over 2 sqrt(k): |d cx| <= 20 u max(1, nnt^2) / (2 cos(t)) + 20 u nnt + 5 u.
    Total internal reflection: exactly where eta sin(i) > 1 from inside, never from outside, outside the band |eta sin(i) - 1| <= 2^-17
    (k = (1 - eta sin i)(1 + eta sin i) is decided by its sign; 20 u eta^2 / 2 < 2^-17 for eta <= 4)."""
    x = _one_bounce(eta, inside)
    nnt = x["nnt"]
    clear = np.abs(x["sin_t"] - 1.0) > 2.0 ** -17
    if inside:
        assert np.array_equal(x["tir"][clear], (x["sin_t"] > 1.0)[clear])
        assert np.count_nonzero(x["tir"]) >= 20 and np.count_nonzero(~x["tir"]) >= 20
    else:
        assert not x["tir"].any()
    ok = ~x["tir"] & clear & (x["sin_t"] < 1.0)
    assert np.array_equal(x["decided"], ~x["tir"])
    snell_bound = (10.0 + 10.0 * max(1.0, nnt * nnt) + 20.0 * nnt) * U
    snell = np.abs(x["sin_t"] - x["sin_t_model"])[ok] / snell_bound
    if inside:
        dcx = 20.0 * U * max(1.0, nnt * nnt) / (2.0 * x["cos_t"][ok]) + 20.0 * U * nnt + 5.0 * U
    else:
        dcx = np.full(np.count_nonzero(ok), 8.0 * U)
    schlick = np.abs(x["re"] - x["schlick"])[ok] / (5.0 * dcx + 12.0 * U)
    print(f"eta {eta} {'inside' if inside else 'outside'}: worst error / bound: Snell {snell.max():.3f}, Schlick {schlick.max():.3f} "
          f"({np.count_nonzero(ok)} angles, {np.count_nonzero(x['tir'])} reflect totally)")
    assert snell.max() <= 1.0 and schlick.max() <= 1.0
    # the arm taken: u_az = 0.5 against P = 0.25 + 0.5 Re -- refracted where Re < 0.5, else (and under total reflection) the mirror direction
    through = x["decided"] & (f32(0.5) >= (f32(0.25) + f32(0.5) * x["re"].astype(f32)))
    for k in range(3):
        assert np.array_equal(x["d_next"][k], np.where(through, x["td"][k], x["m"][k]))


# ---- 4. unbiased choice --------------------------------------------------------------------------------------------------------------
def test_glass_ball_in_the_furnace_returns_the_emission(oracle):
    """A white GLASS 1.5 ball in the furnace: whatever a path does on the ball, its weight has expectation 1 when it reaches the wall,
    so the mean colour over the ball's pixels is E.  16 x 16 pixels, 32 spp, 16 bounces: the reflect arm is chosen with P >= 0.25, so
    a path stays in the ball with about 0.27 per bounce and 0.27^13 = 4e-8 of them could reach the cap; the model counts 0 capped
    paths with weight left out of 8192 (asserted below 1e-3 of all paths: the bias the cap may add).  Standard errors come from
    the pixel means themselves."""
    sph, basis = MC.ball_furnace(), oracle.camera_basis(w=16, h=16)
    img, info = MM.render_frame(16, 16, 32, sph, basis, MM.sincos_of(oracle), [(MC.DIFFUSE, 0.0), (MC.GLASS, 1.5)], max_bounces=16)
    print("glass furnace:", MC.arms(info), "capped with weight", info["capped_live"], "of", info["paths"])
    assert info["capped_live"] < 1e-3 * info["paths"]
    assert min(info[a] for a in ("glass_reflect_front", "glass_reflect_inside", "glass_refract_front", "glass_refract_inside")) >= 20
    on_ball = img[..., 6] == 1.0
    n = np.count_nonzero(on_ball)
    assert n >= 20
    for k in range(3):
        v = img[..., k][on_ball].astype(f64)
        se = v.std(ddof=1) / np.sqrt(n)
        print(f"channel {k}: mean {v.mean():.6f} E {MC.E[k]} standard error {se:.6f} ({(v.mean() - MC.E[k]) / se:+.2f} se, {n} pixels)")
        assert se > 0 and abs(v.mean() - MC.E[k]) <= 4.0 * se
    off = ~on_ball & (img[..., 6] == 0.0)
    assert np.all(img[..., 0][off] == f32(MC.E[0]))


# ---- 5. refusals, header, ABI ---------------------------------------------------------------------------------------------------------
REFUSALS = [
    ([(4, 0.0)], r"table\[0\]\.kind 4 \(0 \.\. 3\)"),
    ([(0, 0.0), (-1, 0.0)], r"table\[1\]\.kind -1"),
    ([(0, 0.5)], r"table\[0\]\.param 0\.5 \(DIFFUSE takes 0\)"),
    ([(1, -0.25)], r"table\[0\]\.param -0\.25 \(MIRROR takes 0\)"),
    ([(2, 0.0)], r"GLOSSY roughness: 0 < rho < 1"),
    ([(2, 1.0)], r"GLOSSY roughness: 0 < rho < 1"),
    ([(2, float("nan"))], r"table\[0\]\.param is not finite"),
    ([(3, 1.0)], r"GLASS index of refraction: 1 < eta <= 4"),
    ([(3, 4.5)], r"GLASS index of refraction: 1 < eta <= 4"),
    ([(3, float("inf"))], r"table\[0\]\.param is not finite"),
    ([(0, float("nan"))], r"table\[0\]\.param is not finite"),
]


@pytest.mark.parametrize("table,message", REFUSALS)
def test_material_check_refuses_by_message(pt, table, message):
    with pytest.raises(pt.PtError, match=message) as e:
        pt.material_check(table)
    assert e.value.code == -1  # PT_EINVAL


def test_material_check_limits_and_accepts(pt):
    pt.material_check(pt.SMALLPT_MATERIALS)
    pt.material_check([pt.Material(pt.MATERIAL_GLOSSY, 0.3), pt.Material(pt.MATERIAL_GLASS, 4.0), pt.Material(pt.MATERIAL_MIRROR)] + [(0, 0.0)] * 61)
    with pytest.raises(pt.PtError, match=r"n 65 exceeds the 64 spheres") as e:
        pt.material_check([(0, 0.0)] * 65)
    assert e.value.code == -5  # PT_ELIMIT
    with pytest.raises(pt.PtError, match=r"pt_material_check: table is NULL"):
        pt.material_check([])
    assert pt.lib.pt_material_check(None, 3) == -1 and b"table is NULL" in pt.lib.pt_last_error()
    assert pt.lib.pt_renderer_set_materials(None, None, 0) == -1 and b"renderer is NULL" in pt.lib.pt_last_error()
    with pytest.raises(ValueError):
        pt.material_check([(0, 0.0, 1.0)])
    with pytest.raises(pt.PtError):  # render_frame checks the table before a renderer -- a device -- exists
        pt.render_frame(8, 8, 1, materials=[(9, 0.0)] * 9)


def test_header_declares_what_the_libraries_export(pt, lab):
    import ctypes

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pt_material_check", "pt_renderer_set_materials"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in pt.ABI and hasattr(ctypes.CDLL(pt.LIB_PATH), name) and hasattr(ctypes.CDLL(lab.LIB_PATH), name)
    values = dict(re.findall(r"\b(PT_MATERIAL_[A-Z]+)\s*=\s*(\d+)", code))
    assert {k: int(v) for k, v in values.items()} == {"PT_MATERIAL_DIFFUSE": pt.MATERIAL_DIFFUSE, "PT_MATERIAL_MIRROR": pt.MATERIAL_MIRROR,
                                                     "PT_MATERIAL_GLOSSY": pt.MATERIAL_GLOSSY, "PT_MATERIAL_GLASS": pt.MATERIAL_GLASS}
    assert int(re.search(r"#define PT_MATERIALS_MAX_SPHERES (\d+)", code).group(1)) == pt.MATERIALS_MAX_SPHERES >= 64
    assert int(re.search(r"#define PT_VARIANT_MATERIALS (\d+)", code).group(1)) == pt.VARIANT_MATERIALS == pt.VARIANT_FAST + 1
    assert pt.MATERIAL_DTYPE.itemsize == 8 and re.search(r"typedef struct pt_material \{\s*int32_t kind;\s*float param;\s*\} pt_material;", code)
    assert pt.lib.pt_abi_version() == 6 and ctypes.sizeof(pt.RendererOpts) == 48
    assert [tuple(m) for m in pt.SMALLPT_MATERIALS] == MC.smallpt()


def test_glass_constants_are_float32(pt):
    inv, r0 = MM.glass_constants(1.5)
    assert inv == f32(1.0) / f32(1.5) and r0 == f32(f32(0.25) / f32(6.25)) and inv.dtype == f32 and r0.dtype == f32


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------
def _cli(*args):
    from conftest import ROOT

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    return subprocess.run([exe, "--size", "16", "-s", "1", "--nobitmap", "--device", "99"] + list(args), capture_output=True, text=True, timeout=60)


CLI_FILES = [
    ("6 shiny\n", r"line 1: kind 'shiny' is none of diffuse, mirror, glossy, glass"),
    ("6\n", r"line 1: expected 'index kind \[param\]'"),
    ("6 glass 1.5 7\n", r"line 1: expected 'index kind \[param\]'"),
    ("6.5 mirror\n", r"line 1: expected 'index kind \[param\]'"),
    ("# nothing\n\n", r"no materials in"),
    ("6 mirror\n9 mirror\n", r"line 2: index 9 outside 0 \.\. 8"),
    ("-1 mirror\n", r"line 1: index -1 outside 0 \.\. 8"),
    ("6 mirror\n6 glass 1.5\n", r"line 2: index 6 is repeated"),
    ("7 glass 1.0\n", r"table\[7\]\.param 1 \(GLASS index of refraction"),
    ("7 glass nan\n", r"table\[7\]\.param is not finite"),
    ("6 mirror 0.5\n", r"table\[6\]\.param 0\.5 \(MIRROR takes 0\)"),
    ("6 glossy\n", r"table\[6\]\.param 0 \(GLOSSY roughness"),
]


@pytest.mark.parametrize("text,message", CLI_FILES)
def test_cli_refuses_a_bad_material_file(tmp_path, text, message):
    f = tmp_path / "materials.txt"
    f.write_text(text)
    res = _cli("--materials", str(f))
    assert res.returncode == 1 and re.search(r"ERROR: --materials: .*" + message, res.stderr), res.stderr
    assert "GPUassert" not in res.stderr  # refused before a device was touched


@pytest.mark.parametrize("extra,other", [(["--progressive", "2"], "--progressive"), (["--poses", "x", "--batch"], "--batch"), (["--gpus", "2"], "--gpus")])
def test_cli_refuses_combinations_before_a_device(extra, other):
    res = _cli("--materials", "smallpt", *extra)
    assert res.returncode == 1 and f"--materials cannot be combined with {other}" in res.stderr and "GPUassert" not in res.stderr, res.stderr


def test_cli_reads_a_good_file_and_the_preset(tmp_path):
    """A good table passes every host check: the run then stops at the device it was told to use (--device 99), not before."""
    f = tmp_path / "materials.txt"
    f.write_text("# smallpt's balls\n6 mirror\n7 glass 1.5\n8 0\n3 glossy 0.25\n")
    for arg in (str(f), "smallpt"):
        res = _cli("--materials", arg)
        assert res.returncode != 0 and "GPUassert:" in res.stderr and "--materials" not in res.stderr, res.stderr
    res = _cli("--materials", "smallpt", "--spheres", "12")
    assert res.returncode == 1 and "smallpt preset is for the reference's scene of 9 spheres" in res.stderr
    res = _cli("--materials", str(tmp_path / "missing.txt"))
    assert res.returncode == 1 and "cannot open material file" in res.stderr
    res = _cli("--materials")
    assert res.returncode == 1 and "required argument for option '--materials' is missing" in res.stderr
