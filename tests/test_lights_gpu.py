"""Direct light sampling on the device (the LIGHTS build of csrc/pt_materials.hip, PT_VARIANT_MATERIALS_LIGHTS): every frame bit for
bit, all 14 channels, against tests/lights_model.py, the definition in NumPy float32 (EXACTNESS.md A.23), and against the oracle
where no light is ever sampled.

The 24 x 24 model frames of a table of cases are computed once and shared.  Counters first: a case compares bits only after the
model has shown that the frame exercises what the case claims -- every counter it names >= 20 in that frame, or, at 1 spp, >= 20
over the cases of its table and > 0 in the frame itself (as tests/test_materials_gpu.py does)."""
import os
import subprocess

import numpy as np
import pytest

import lights_cases as LC
import lights_model as LM
import materials_cases as MC
import materials_model as MM

pytestmark = pytest.mark.gpu

RNGS = {"xorwow": 0, "philox": 1}
FLOOR = 20


def _model(oracle, size, spp, spheres, basis, materials=None, rng="xorwow", **kw):
    return LM.render_frame(size, size, spp, spheres, basis, MM.sincos_of(oracle), materials, rng=rng, philox=oracle.philox, **kw)


def _exercised(info, total, named, spp, what):
    """The cap: each named counter >= FLOOR in the frame; at 1 spp >= FLOOR over the table's cases and > 0 in the frame."""
    got = {c: info[c] for c in named}
    print(f"{what}: {LC.counters(info)} arms {MC.arms(info)} lit per light {info['lit_per_light']}; over the table's cases {total}")
    if spp == 1:
        assert min(total[c] for c in named) >= FLOOR and min(got.values()) > 0, (got, total)
    else:
        assert min(got.values()) >= FLOOR, got


class _Session:
    """A renderer with light sampling on, its scene and its frame buffer."""

    def __init__(self, pt, size, spp, spheres, materials=None, rows=None, lights=True, **opts):
        self.pt, self.size = pt, size
        if rows:
            opts.update(row_begin=rows[0], row_end=rows[1])
        self.r = pt.Renderer(size, size, spp, **opts)
        self.d_scene, self.n = pt.upload_scene(spheres)
        self.d_out = pt.DeviceBuffer(max(self.r.tile_floats * 4, 4))
        if materials is not None:
            self.r.set_materials(materials)
        if lights:
            self.r.set_light_sampling(True)

    def frame(self, basis, eye=LC.EYE):
        self.r.render(self.d_out.ptr, self.d_scene.ptr, self.n, basis, eye)
        return self.d_out.download(np.float32, (self.r.rows, self.size, 14))

    def close(self):
        self.d_out.free()
        self.d_scene.free()
        self.r.destroy()


def _xorwow_of(words, rows, width):
    import numpy_restatement as NR

    g = NR.Xorwow(np.zeros((rows, width), dtype=np.uint64))
    g.d = words[:, 0].reshape(rows, width).copy()
    g.v = [words[:, 1 + k].reshape(rows, width).copy() for k in range(5)]
    return g


def _words_of(g):
    return np.stack([g.d.reshape(-1)] + [v.reshape(-1) for v in g.v], axis=1).astype(np.uint32)


# ---- 1. the small-lamp box ----------------------------------------------------------------------------------------------------------------
# What the model counts in this scene decides what a case may name.  The lamp has radius 1.5: at 24 x 24 a frame of 4 spp and 8
# bounces holds 2 .. 5 `suppressed` hits (a bounce lands on it with 1e-3), 0 or 1 `kept` (a mirror or glass bounce lands on it with
# 3e-4, and no frame this small shows 20 pixel samples of its reflection), and with SMALLPT_MATERIALS no `below` at all: every
# DIFFUSE surface of the closed box faces the lamp, only the two balls have a far side, and they are the mirror and the glass.
# So this table names `sampled`, `lit`, `shadowed` (and `below` with the all-diffuse table, every arm of A.22 with the materials),
# and the three counters it cannot reach have cases of their own below: `suppressed` in this same scene from a camera under the
# lamp, `kept` and a lamp reached through the mirror or the glass (and `below` with materials) in the reference's box, whose lamp
# the balls do show.  The two arms of A.22 that SMALLPT_MATERIALS does not have follow: `glossy` (both balls GLOSSY) and `tir`
# (the eye inside a glass sphere), each with the lamp kept after it.
BOX_CASES = [(spp, mb, rng) for spp in (4, 1) for mb in (5, 8) for rng in sorted(RNGS)]
DIRECT = ("sampled", "lit", "shadowed", "below")
ARMS = ("diffuse", "mirror", "glass_reflect_front", "glass_reflect_inside", "glass_refract_front", "glass_refract_inside")
SPECULAR = ("sampled", "lit", "shadowed") + ARMS


@pytest.fixture(scope="module")
def box_models(oracle):
    """{with materials: {(spp, max_bounces, rng): (frame, info)}} of the small-lamp box at 24 x 24, computed once."""
    sph, basis = LC.small_lamp_box(oracle.scene_cornell()), oracle.camera_basis(w=24, h=24)
    return {mats: {(spp, mb, rng): _model(oracle, 24, spp, sph, basis, MC.smallpt() if mats else None, rng, max_bounces=mb)
                   for spp, mb, rng in BOX_CASES} for mats in (False, True)}


@pytest.mark.parametrize("spp,mb,rng", BOX_CASES)
@pytest.mark.parametrize("mats", [False, True])
def test_small_lamp_box_equals_the_model(pt, oracle, gpu, box_models, mats, spp, mb, rng):
    named = SPECULAR if mats else DIRECT
    total = {c: sum(info[c] for _, info in box_models[mats].values()) for c in named}
    want, info = box_models[mats][(spp, mb, rng)]
    _exercised(info, total, named, spp, f"small-lamp box materials={mats} {spp} spp {mb} bounces {rng}")
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(width=24, height=24)
    assert np.array_equal(basis, oracle.camera_basis(w=24, h=24))
    img, _ = pt.render_frame(24, 24, spp, sph, basis, materials=pt.SMALLPT_MATERIALS if mats else None, light_sampling=True, max_bounces=mb,
                             rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"small-lamp box materials={mats} {spp} spp {mb} bounces {rng}")


UNDER_THE_LAMP = ((50.0, 55.0, 81.6), -90.0, 89.0)  # eye, yaw, pitch: ten units under the lamp, looking up at it and the ceiling


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("mats", [False, True])
def test_small_lamp_box_from_under_the_lamp_leaves_out_what_was_sampled(pt, oracle, gpu, mats, rng):
    """`suppressed`: first hits on the ceiling around the lamp, whose next bounce lands on the lamp they have just sampled."""
    eye, yaw, pitch = UNDER_THE_LAMP
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(eye, yaw, pitch, width=32, height=32)
    assert np.array_equal(basis, oracle.camera_basis(eye, yaw, pitch, w=32, h=32))
    want, info = _model(oracle, 32, 4, sph, basis, MC.smallpt() if mats else None, rng, eye=eye)
    _exercised(info, None, ("suppressed", "self", "sampled", "lit"), 4, f"under the lamp materials={mats} {rng}")
    img, _ = pt.render_frame(32, 32, 4, sph, basis, eye, materials=pt.SMALLPT_MATERIALS if mats else None, light_sampling=True, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"under the lamp materials={mats} {rng}")


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_a_lamp_seen_in_the_mirror_and_through_the_glass_keeps_its_light(pt, oracle, gpu, rng):
    """`kept`: the reference's box with SMALLPT_MATERIALS, 8 bounces.  A hit on the lamp after a MIRROR or GLASS bounce was not
    sampled by the previous hit and adds its emission; after a DIFFUSE bounce it is `suppressed`."""
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=32, height=32)
    want, info = _model(oracle, 32, 4, sph, basis, MC.smallpt(), rng, max_bounces=8)
    _exercised(info, None, ("kept", "kept_after_specular", "suppressed", "below", "sampled", "lit") + ARMS, 4, f"lamp in the mirror {rng}")
    img, _ = pt.render_frame(32, 32, 4, sph, basis, materials=pt.SMALLPT_MATERIALS, light_sampling=True, max_bounces=8, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"lamp in the mirror {rng}")


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_glossy_balls_never_sample_and_keep_the_lamps_light(pt, oracle, gpu, rng):
    """The `glossy` arm, and A.23's one decision about it: GLOSSY carries no pdf, so it is treated as specular -- a GLOSSY hit takes
    the light draws, forms no sample and marks nothing, and a lamp hit after it keeps its emission (`kept_after_glossy`).  The
    reference's box with both balls GLOSSY 0.3, 8 bounces."""
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=24, height=24)
    want, info = _model(oracle, 24, 4, sph, basis, LC.GLOSSY_BALLS, rng, max_bounces=8)
    _exercised(info, None, ("glossy", "kept", "kept_after_glossy", "suppressed", "below", "sampled", "lit", "diffuse"), 4, f"glossy balls {rng}")
    assert info["mirror"] == 0 and info["kept_after_specular"] == info["kept_after_glossy"]
    img, _ = pt.render_frame(24, 24, 4, sph, basis, materials=LC.GLOSSY_BALLS, light_sampling=True, max_bounces=8, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"glossy balls {rng}")


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_total_internal_reflection_with_a_lamp_equals_the_model(pt, oracle, gpu, rng):
    """The `tir` arm: the eye inside a glass sphere, a lamp seen through the glass where the rays leave it."""
    sph, basis = LC.glass_around_the_eye(), pt.camera_basis(width=24, height=24)
    want, info = _model(oracle, 24, 4, sph, basis, LC.GLASS_AROUND_THE_EYE_TABLE, rng, max_bounces=8)
    _exercised(info, None, ("tir", "glass_refract_inside", "glass_reflect_inside", "kept", "kept_after_specular", "suppressed", "sampled", "lit"), 4,
               f"glass around the eye {rng}")
    img, _ = pt.render_frame(24, 24, 4, sph, basis, materials=LC.GLASS_AROUND_THE_EYE_TABLE, light_sampling=True, max_bounces=8, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"glass around the eye {rng}")


# ---- 1b. the closed form on the device ---------------------------------------------------------------------------------------------------
def test_floor_under_a_small_lamp_is_the_closed_form_on_the_device(pt, oracle, gpu):
    """tests/test_lights_host.py's closed form, held against the DEVICE's frame: floor and lamp, 1 spp, max_bounces = 2, every floor
    pixel inside albedo * Le * 2 vers * [cos(theta + a), cos(max(theta - a, 0))] widened by 64 float32 roundings -- and almost none
    of them with the option off.  Nothing of the model takes part in the bound."""
    size = 24
    sph = LC.floor_and_lamp()
    basis = pt.camera_basis(LC.FLOOR_EYE, LC.FLOOR_YAW, LC.FLOOR_PITCH, width=size, height=size)
    img, _ = pt.render_frame(size, size, 1, sph, basis, LC.FLOOR_EYE, light_sampling=True, max_bounces=2)
    off, _ = pt.render_frame(size, size, 1, sph, basis, LC.FLOOR_EYE, max_bounces=2)
    covered, passed, widest = LC.floor_closed_form(img, basis, size)
    _, passed_off, _ = LC.floor_closed_form(off, basis, size)
    print(f"closed form on the device: {covered} floor pixels, {passed} inside (option off: {passed_off}); widest interval {widest:.5f} of the scale")
    assert covered >= 200 and widest < 0.01
    assert passed == covered
    assert passed_off < 0.05 * covered
    want, _ = _model(oracle, size, 1, sph, basis, None, eye=LC.FLOOR_EYE, max_bounces=2)
    LC.assert_same_bits(img, want, "floor and lamp")


# ---- 2. three lamps: self, every lamp lit, Philox blocks with word 3 = 2 -------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_three_lamp_box_equals_the_model(pt, oracle, gpu, rng):
    sph, basis = LC.three_lamp_box(pt.scene_cornell()), pt.camera_basis(width=24, height=24)
    want, info = _model(oracle, 24, 4, sph, basis, None, rng)
    _exercised(info, None, ("self", "sampled", "lit", "suppressed"), 4, f"three-lamp box {rng}")
    assert info["lights"] == [8, 9, 10] and min(info["lit_per_light"]) >= FLOOR, info["lit_per_light"]
    img, _ = pt.render_frame(24, 24, 4, sph, basis, light_sampling=True, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"three-lamp box {rng}")


# ---- 3. the reference's box: the lamp sphere reaches through the ceiling -------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_reference_box_equals_the_model(pt, oracle, gpu, rng):
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=24, height=24)
    want, info = _model(oracle, 24, 4, sph, basis, None, rng)
    _exercised(info, None, ("sampled", "lit", "shadowed", "suppressed"), 4, f"the reference's box {rng}")
    img, _ = pt.render_frame(24, 24, 4, sph, basis, light_sampling=True, rng_mode=RNGS[rng])
    LC.assert_same_bits(img, want, f"the reference's box {rng}")


# ---- 4. anchors: nothing to sample -> the oracle's frame -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["no light", "one bounce"])
def test_anchors_equal_the_oracle_with_persisted_state(pt, oracle, gpu, what):
    size, spp = 24, 4
    box, basis = pt.scene_cornell(), pt.camera_basis(width=size, height=size)
    sph, mb = (LC.no_light_box(box), 5) if what == "no light" else (LC.small_lamp_box(box), 1)
    s = _Session(pt, size, spp, sph, max_bounces=mb)
    assert s.r.kernel_info(9)["variant"] == pt.VARIANT_MATERIALS_LIGHTS
    st = oracle.setup_random(size, size)
    for frame in range(2):
        ref = oracle.render(size, size, spp, spheres=sph, basis=basis, rng_state=st, max_bounces=mb)
        LC.assert_same_bits(s.frame(basis), ref, f"{what}, frame {frame}")
        assert np.array_equal(s.r.get_rng_state(), st)
    s.close()


# ---- 5. persisted XORWOW with lights -------------------------------------------------------------------------------------------------------
def test_persisted_xorwow_state_follows_the_model_over_two_frames(pt, oracle, gpu):
    size, spp = 24, 1
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(width=size, height=size)
    s = _Session(pt, size, spp, sph, pt.SMALLPT_MATERIALS)
    state = _xorwow_of(oracle.setup_random(size, size), size, size)
    sampled = 0
    for frame in range(2):
        want, info = _model(oracle, size, spp, sph, basis, MC.smallpt(), state=state)
        sampled += info["sampled"]
        LC.assert_same_bits(s.frame(basis), want, f"persisted state, frame {frame}")
        state = info["state"]
        assert np.array_equal(s.r.get_rng_state(), _words_of(state)), frame
    assert sampled >= FLOOR
    s.close()


# ---- 6. row tile, planar layout, display vertices -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_row_tile_equals_the_models_rows(pt, oracle, gpu, box_models, rng):
    want, info = box_models[True][(4, 5, rng)]
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(width=24, height=24)
    rows, rinfo = _model(oracle, 24, 4, sph, basis, MC.smallpt(), rng, row_begin=8, row_end=16)
    assert rinfo["sampled"] >= FLOOR and rinfo["lit"] >= FLOOR
    LC.assert_same_bits(rows, want[8:16], "the model's rows [8, 16)")  # both generators are keyed on the pixel's id
    tile, _ = pt.render_frame(24, 24, 4, sph, basis, materials=pt.SMALLPT_MATERIALS, light_sampling=True, rng_mode=RNGS[rng], row_begin=8, row_end=16)
    LC.assert_same_bits(tile, rows, f"rows [8, 16) of 24 {rng}")


def test_planar_layout_and_display_vertices_hold_the_same_frame(pt, gpu, box_models):
    want, info = box_models[True][(4, 5, "xorwow")]
    assert info["lit"] >= FLOOR
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(width=24, height=24)
    s = _Session(pt, 24, 4, sph, pt.SMALLPT_MATERIALS, layout=pt.LAYOUT_PLANAR, persist_rng=False)
    d_vtx = pt.DeviceBuffer(24 * 24 * 3 * 4)
    s.r.set_display(d_vtx.ptr)
    s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    planar = s.d_out.download(np.float32, (14, 24, 24))
    vtx = d_vtx.download(np.float32, (24, 24, 3))
    d_vtx.free()
    s.close()
    LC.assert_same_bits(np.ascontiguousarray(planar.transpose(1, 2, 0)), want, "planar layout")
    LC.assert_same_bits(vtx, pt.display_pack(want), "display vertices")


# ---- 7. on and off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mats", [False, True])
def test_switching_off_returns_the_renderer_to_what_it_was(pt, oracle, gpu, mats):
    size, spp = 24, 4
    sph, basis = LC.small_lamp_box(pt.scene_cornell()), pt.camera_basis(width=size, height=size)
    table = pt.SMALLPT_MATERIALS if mats else None
    s = _Session(pt, size, spp, sph, table, lights=False, persist_rng=False)
    before = s.r.kernel_info(9)["variant"]
    assert before == (pt.VARIANT_MATERIALS if mats else before) and before != pt.VARIANT_MATERIALS_LIGHTS
    old = s.frame(basis)
    s.r.set_light_sampling(True)
    info = s.r.kernel_info(9)
    print(f"kernel_info with light sampling: {info}")
    assert info["variant"] == pt.VARIANT_MATERIALS_LIGHTS and info["scratch_bytes"] == 0 and info["num_vgprs"] <= 128
    want, minfo = _model(oracle, size, spp, sph, basis, MC.smallpt() if mats else None)
    assert minfo["lit"] >= FLOOR
    LC.assert_same_bits(s.frame(basis), want, "switched on")
    s.r.set_light_sampling(False)
    assert s.r.kernel_info(9)["variant"] == before
    LC.assert_same_bits(s.frame(basis), old, "switched off: the old bits")
    if mats:  # the order of the two calls does not matter
        s.r.set_materials(None)
        s.r.set_light_sampling(True)
        s.r.set_materials(table)
        LC.assert_same_bits(s.frame(basis), want, "light sampling first, the table second")
    s.close()


# ---- 8. many spheres -------------------------------------------------------------------------------------------------------------------------
def test_twelve_random_spheres_with_two_lamps_equal_the_model(pt, oracle, gpu):
    """Twelve spheres: past PT_SCREEN_MAX_SPHERES the search, the shadow ray's too, takes its many-sphere path."""
    sph, basis = LC.two_lamps_among_twelve(pt.scene_random(12, seed=3, with_walls=True)), pt.camera_basis(width=24, height=24)
    want, info = _model(oracle, 24, 4, sph, basis, None, max_bounces=4)
    _exercised(info, None, ("sampled", "lit", "shadowed"), 4, "twelve spheres, two lamps")
    assert len(info["lights"]) == 2 and min(info["lit_per_light"]) >= FLOOR
    img, _ = pt.render_frame(24, 24, 4, sph, basis, light_sampling=True, max_bounces=4)
    LC.assert_same_bits(img, want, "twelve spheres, two lamps")


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_launch_nothing(pt, gpu):
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=16, height=16)
    for opts, msg in ((dict(fast_math=True), r"pt_renderer_set_light_sampling: a fast_math renderer has no light sampling"),
                      (dict(variant=6), r"pt_renderer_set_light_sampling: the renderer has an explicit kernel variant \(6\)")):
        r = pt.Renderer(16, 16, 1, **opts)
        with pytest.raises(pt.PtError, match=msg) as e:
            r.set_light_sampling(True)
        assert e.value.code == -1
        r.set_light_sampling(False)  # switching off what is off is no error
        r.destroy()
    s = _Session(pt, 16, 1, sph)
    sentinel = np.full(16 * 16 * 14, 12345.0, dtype=np.float32)
    with pytest.raises(pt.PtError, match=r"pt_progressive_create: the renderer samples its lights directly \(pt_renderer_set_light_sampling\)"):
        pt.Progressive(s.r)
    d_two = pt.DeviceBuffer(2 * s.r.tile_floats * 4)
    d_two.upload(np.concatenate([sentinel, sentinel]))
    with pytest.raises(pt.PtError, match=r"pt_renderer_enqueue_frames: the renderer samples its lights directly"):
        s.r.enqueue_frames(d_two.ptr, s.r.tile_floats, s.d_scene.ptr, s.n, [basis, basis], [LC.EYE, LC.EYE])
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(d_two.download(np.float32, (2 * sentinel.size,)), np.concatenate([sentinel, sentinel]))
    d_two.free()
    s.r.set_light_sampling(False)
    p = pt.Progressive(s.r)  # a session made while the option was off refuses its passes while it is on
    s.r.set_light_sampling(True)
    with pytest.raises(pt.PtError, match=r"pt_progressive: the renderer samples its lights directly"):
        p.render(1, s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    p.destroy()
    s.close()
    # without a table a scene above PT_MATERIALS_MAX_SPHERES is PT_ELIMIT, by name, and nothing is launched
    big = pt.scene_random(65, seed=5, with_walls=True)
    s = _Session(pt, 16, 1, big)
    s.d_out.upload(sentinel)
    with pytest.raises(pt.PtError, match=r"render: 65 spheres exceed the 64 spheres \(PT_MATERIALS_MAX_SPHERES\)") as e:
        s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    assert e.value.code == -5  # PT_ELIMIT
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(s.d_out.download(np.float32, sentinel.shape), sentinel)
    s.close()


# ---- 10. command line -------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_librarys_frame(pt, gpu, tmp_path):
    from conftest import ROOT
    from test_parity_gpu import _read_feature_exr

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    out = str(tmp_path / "box")
    res = subprocess.run([exe, "--size", "32", "-s", "4", "--materials", "smallpt", "--direct-light", "--nobitmap", "-o", out], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    img, _ = pt.render_frame(32, 32, 4, materials=pt.SMALLPT_MATERIALS, light_sampling=True, basis=pt.camera_basis(width=32, height=32))
    names, planes = _read_feature_exr(out + ".exr")
    src = {"Color.R": 0, "Color.G": 1, "Color.B": 2, "Normal.X": 3, "Normal.Y": 4, "Normal.Z": 5, "Albedo.R": 6, "Albedo.G": 7, "Albedo.B": 8,
           "Depth.Z": 9, "ColorVar.Z": 10, "NormalVar.Z": 11, "AlbedoVar.Z": 12, "DepthVar.Z": 13}
    assert len(names) == 14
    for k, nm in enumerate(names):
        assert np.array_equal(planes[k].view(np.uint32), img[..., src[nm]].view(np.uint32)), nm
    plain, _ = pt.render_frame(32, 32, 4, materials=pt.SMALLPT_MATERIALS, basis=pt.camera_basis(width=32, height=32))
    assert not np.array_equal(plain[..., :3], img[..., :3])
