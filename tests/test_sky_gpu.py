"""Sky and sun on the device (the SKY builds of csrc/pt_materials.hip, PT_VARIANT_MATERIALS_SKY / PT_VARIANT_MATERIALS_LIGHTS_SKY): every
frame bit for bit, all 14 channels, against tests/sky_model.py, the definition in NumPy float32 (EXACTNESS.md A.24), against closed
forms that do not come from the model, and against the oracle where no ray leaves the scene.

Counters first, as in tests/test_lights_gpu.py: a case compares bits only after the model has shown that the frame exercises what
the case names -- every named counter >= 20 in that frame, or, at 1 spp, >= 20 over the 1-spp cases of its table that share its
sky, table and option, and > 0 in the frame itself.  A model frame is computed once per module and shared."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import materials_cases as MC
import materials_model as MM
import sky_cases as SC
import sky_model as SM

pytestmark = pytest.mark.gpu

RNGS = {"xorwow": 0, "philox": 1}
FLOOR = 20
SIZE = 24
_MODELS = {}


def _model(oracle, key, size, spp, spheres, basis, sky, materials=None, light_sampling=False, rng="xorwow", **kw):
    """The model's (frame, info), computed once per module under `key`."""
    if key not in _MODELS:
        _MODELS[key] = SM.render_frame(size, size, spp, spheres, basis, MM.sincos_of(oracle), sky, materials, light_sampling=light_sampling, rng=rng,
                                       philox=oracle.philox, **kw)
    return _MODELS[key]


def _exercised(info, total, named, spp, what):
    got = {c: info[c] for c in named}
    print(f"{what}: {SC.counters(info)} arms {MC.arms(info)}; over the table's 1-spp cases {total}")
    if spp == 1:
        assert min(total[c] for c in named) >= FLOOR and min(got.values()) > 0, (got, total)
    else:
        assert min(got.values()) >= FLOOR, got


class _Session:
    """A renderer, its scene and its frame buffer."""

    def __init__(self, pt, size, spp, spheres, rows=None, **opts):
        self.pt, self.size = pt, size
        if rows:
            opts.update(row_begin=rows[0], row_end=rows[1])
        self.r = pt.Renderer(size, size, spp, **opts)
        self.d_scene, self.n = pt.upload_scene(spheres)
        self.d_out = pt.DeviceBuffer(max(self.r.tile_floats * 4, 4))

    def frame(self, basis, eye=SC.EYE):
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


# ---- 1. the courtyard against the model -----------------------------------------------------------------------------------------------------
# What the model counts decides what a case may name (24 x 24; the figures are the model's own, XORWOW, 4 spp and 1 spp):
#   every case            escaped_primary 1436 / 360, escaped_later 760-860 / 190-212, up, ground 240 / 50
#   sampling on           sun_sampled 760-1004 / 188-244, sun_lit 580-905 / 145-217
#   sun_shadowed          small 21-36 / 7-11, wide 21-38 / 6-10, low 35-51 / 8-15, in view 180-212 / 43-49
#   sun_below             all-diffuse: small 26-67 / 5-16, wide 23-61 / 8-19, low 155-195 / 37-47, in view 108-154 / 28-37;
#                         with the mirror and the glass only the low sun has any (132-140 / 30-33): the far side of the floor is the
#                         horizon, and the balls are the two spheres with a far side
#   sun_suppressed        wide 101-119 / 21-29, low 40-49 / 14-21; the small sun 0-2: a bounce enters a cone of 0.006 sr twice in a thousand
#   sun_kept              sampling off: wide 114-133 / 21-24 (later escapes); in view 233-238 / 56-58 (primary rays, on or off)
# sun_kept_after_specular has a case of its own below (a camera close to the mirror ball).
SUN_NAMES = ("small", "wide", "low", "in view")
COURTYARD_CASES = list(itertools.product((4, 1), (5, 2), sorted(RNGS), (False, True), (False, True), SUN_NAMES))  # spp, bounces, rng, mats, sampling, sun
ESCAPES = ("escaped_primary", "escaped_later", "up", "ground")


def _named(mats, sampling, sun):
    named = ESCAPES
    if sampling:
        named += ("sun_sampled", "sun_lit", "sun_shadowed")
        if not mats or sun == "low":
            named += ("sun_below",)
        if sun in ("wide", "low"):
            named += ("sun_suppressed",)
    if sun == "in view" or (sun == "wide" and not sampling):
        named += ("sun_kept",)
    return named


def _courtyard_model(oracle, spp, mb, rng, mats, sampling, sun):
    sph, basis = SC.courtyard(oracle.scene_cornell()), oracle.camera_basis(w=SIZE, h=SIZE)
    return _model(oracle, ("courtyard", spp, mb, rng, mats, sampling, sun), SIZE, spp, sph, basis, SC.SUNS[sun], SC.COURTYARD_SMALLPT if mats else None,
                  sampling, rng, max_bounces=mb)


@pytest.mark.parametrize("spp,mb,rng,mats,sampling,sun", COURTYARD_CASES)
def test_courtyard_equals_the_model(pt, oracle, gpu, spp, mb, rng, mats, sampling, sun):
    named = _named(mats, sampling, sun)
    want, info = _courtyard_model(oracle, spp, mb, rng, mats, sampling, sun)
    total = None
    if spp == 1:
        siblings = [_courtyard_model(oracle, 1, b, g, mats, sampling, sun)[1] for b in (5, 2) for g in sorted(RNGS)]
        total = {c: sum(i[c] for i in siblings) for c in named}
    what = f"courtyard, {sun} sun, materials={mats} sampling={sampling} {spp} spp {mb} bounces {rng}"
    _exercised(info, total, named, spp, what)
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    assert np.array_equal(basis, oracle.camera_basis(w=SIZE, h=SIZE))
    img, _ = pt.render_frame(SIZE, SIZE, spp, sph, basis, materials=SC.COURTYARD_SMALLPT if mats else None, light_sampling=sampling,
                             sky=SC.to_pt(pt, SC.SUNS[sun]), max_bounces=mb, rng_mode=RNGS[rng])
    SC.assert_same_bits(img, want, what)


MIRROR_EYE, MIRROR_YAW, MIRROR_PITCH = (43.0, 48.5, 65.0), -131.6, -53.0  # 40 units from the mirror ball towards the sun, looking back at it


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_a_sun_seen_in_the_mirror_keeps_its_light(pt, oracle, gpu, rng):
    """`sun_kept_after_specular`: the wide sun stands behind the camera and the mirror ball shows it; a MIRROR hit samples nothing, so
    the escape after it takes the disc, while the floor around the ball samples the sun and its next escape does not."""
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(MIRROR_EYE, MIRROR_YAW, MIRROR_PITCH, width=SIZE, height=SIZE)
    assert np.array_equal(basis, oracle.camera_basis(MIRROR_EYE, MIRROR_YAW, MIRROR_PITCH, w=SIZE, h=SIZE))
    want, info = _model(oracle, ("mirror", rng), SIZE, 4, sph, basis, SC.SUNS["wide"], SC.COURTYARD_SMALLPT, True, rng, eye=MIRROR_EYE)
    _exercised(info, None, ("sun_kept", "sun_kept_after_specular", "sun_suppressed", "sun_sampled", "sun_lit", "sun_shadowed", "mirror"), 4,
               f"sun in the mirror {rng}")
    assert info["sun_kept"] == info["sun_kept_after_specular"]
    img, _ = pt.render_frame(SIZE, SIZE, 4, sph, basis, MIRROR_EYE, materials=SC.COURTYARD_SMALLPT, light_sampling=True, sky=SC.to_pt(pt, SC.SUNS["wide"]),
                             rng_mode=RNGS[rng])
    SC.assert_same_bits(img, want, f"sun in the mirror {rng}")


# ---- 2. closed forms on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("yaw,pitch", SC.ESCAPE_VIEWS)
def test_every_primary_ray_escapes_is_the_sky_itself_on_the_device(pt, gpu, yaw, pitch, sampling):
    sky = SC.SUNS["in view"]
    basis = pt.camera_basis(SC.EYE, yaw, pitch, width=SIZE, height=SIZE)
    img, _ = pt.render_frame(SIZE, SIZE, 1, SC.behind_the_camera(), basis, sky=SC.to_pt(pt, sky), light_sampling=sampling)
    n_up, n_down, n_sun = SC.assert_escape_frame(img, basis, SIZE, sky, f"view {yaw} {pitch}")
    print(f"view {yaw} {pitch}: {n_up} pixels above the horizon, {n_down} below, {n_sun} inside the sun's cone")


@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("sampling", [False, True])
def test_furnace_ball_under_a_uniform_sky_is_a_quarter_on_the_device(pt, gpu, sampling, rng):
    img, _ = pt.render_frame(SIZE, SIZE, 4, SC.furnace_ball(), pt.camera_basis(width=SIZE, height=SIZE), sky=SC.to_pt(pt, SC.FURNACE_SKY),
                             light_sampling=sampling, max_bounces=3, rng_mode=RNGS[rng])
    whole = SC.assert_furnace_frame(img, f"furnace (device) sampling={sampling} {rng}")
    print(f"furnace on the device: {whole} pixels wholly on the ball")


def test_sun_on_a_floor_is_the_closed_form_on_the_device(pt, oracle, gpu):
    """tests/test_sky_host.py's closed form (c), held against the DEVICE's frame; nothing of the model takes part in the bound."""
    basis = pt.camera_basis(SC.SUN_FLOOR_EYE, SC.SUN_FLOOR_YAW, SC.SUN_FLOOR_PITCH, width=SIZE, height=SIZE)
    sky = SC.to_pt(pt, SC.SUN_FLOOR_SKY)
    img, _ = pt.render_frame(SIZE, SIZE, 1, SC.floor_only(), basis, SC.SUN_FLOOR_EYE, sky=sky, light_sampling=True, max_bounces=2)
    off, _ = pt.render_frame(SIZE, SIZE, 1, SC.floor_only(), basis, SC.SUN_FLOOR_EYE, sky=sky, max_bounces=2)
    covered, passed, widest = SC.sun_floor_closed_form(img, basis, SIZE)
    _, passed_off, _ = SC.sun_floor_closed_form(off, basis, SIZE)
    print(f"sun on a floor, device: {covered} floor pixels, {passed} inside (sampling off: {passed_off}); widest interval {widest:.5f} of the scale")
    assert covered >= 500 and widest < 0.01
    assert passed == covered
    assert passed_off < 0.05 * covered
    want, _ = _model(oracle, "sun floor", SIZE, 1, SC.floor_only(), basis, SC.SUN_FLOOR_SKY, None, True, eye=SC.SUN_FLOOR_EYE, max_bounces=2)
    SC.assert_same_bits(img, want, "sun on a floor")


# ---- 3. anchors on the device ----------------------------------------------------------------------------------------------------------------
def test_closed_box_under_a_sky_is_the_oracles_frame_with_persisted_state(pt, oracle, gpu):
    size, spp = SIZE, 4
    box, basis = pt.scene_cornell(), pt.camera_basis(width=size, height=size)
    s = _Session(pt, size, spp, box)
    s.r.set_sky(pt.CLEAR_SKY)
    assert s.r.kernel_info(9)["variant"] == pt.VARIANT_MATERIALS_SKY
    st = oracle.setup_random(size, size)
    for frame in range(2):
        ref = oracle.render(size, size, spp, spheres=box, basis=basis, rng_state=st)
        SC.assert_same_bits(s.frame(basis), ref, f"closed box under a sky, frame {frame}")
        assert np.array_equal(s.r.get_rng_state(), st)
    s.close()


@pytest.mark.parametrize("mats,sampling", [(False, False), (True, False), (False, True), (True, True)])
def test_clearing_the_sky_returns_the_renderer_to_what_it_was(pt, oracle, gpu, mats, sampling):
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)

    def fresh():
        s = _Session(pt, SIZE, 4, sph)
        if mats:
            s.r.set_materials(SC.COURTYARD_SMALLPT)
        if sampling:
            s.r.set_light_sampling(True)
        return s

    plain, s = fresh(), fresh()
    before = s.r.kernel_info(3)["variant"]
    assert before not in (pt.VARIANT_MATERIALS_SKY, pt.VARIANT_MATERIALS_LIGHTS_SKY)
    first = plain.frame(basis)
    SC.assert_same_bits(s.frame(basis), first, "before the sky")
    s.r.set_sky(SC.to_pt(pt, SC.SUNS["wide"]))
    assert s.r.kernel_info(3)["variant"] == (pt.VARIANT_MATERIALS_LIGHTS_SKY if sampling else pt.VARIANT_MATERIALS_SKY)
    state = _xorwow_of(plain.r.get_rng_state(), SIZE, SIZE)
    want, info = SM.render_frame(SIZE, SIZE, 4, sph, basis, MM.sincos_of(oracle), SC.SUNS["wide"], SC.COURTYARD_SMALLPT if mats else None,
                                 light_sampling=sampling, state=state)
    assert info["escaped_later"] >= FLOOR
    SC.assert_same_bits(s.frame(basis), want, "under the sky, second frame of the persisted stream")
    s.r.set_sky(None)
    after = s.r.kernel_info(3)["variant"]
    if mats or sampling:
        assert after == before
    else:  # the automatic choice among the table's variants may move from frame to frame; it is one of them again
        assert 0 <= after < pt.VARIANT_FAST
    # the renderer that never saw a sky renders the same two frames: the second with the sky's stream set into it
    plain.r.set_rng_state(s.r.get_rng_state())
    SC.assert_same_bits(s.frame(basis), plain.frame(basis), "cleared: the frame of a renderer that never had a sky")
    assert np.array_equal(s.r.get_rng_state(), plain.r.get_rng_state())
    plain.close()
    s.close()


def test_all_orders_of_the_three_setters_give_the_same_frame(pt, oracle, gpu):
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    want, info = _courtyard_model(oracle, 4, 5, "xorwow", True, True, "wide")
    assert info["sun_lit"] >= FLOOR and info["mirror"] >= FLOOR
    sky = SC.to_pt(pt, SC.SUNS["wide"])
    for order in itertools.permutations("mls"):
        s = _Session(pt, SIZE, 4, sph, persist_rng=False)
        for c in order:
            {"m": lambda: s.r.set_materials(SC.COURTYARD_SMALLPT), "l": lambda: s.r.set_light_sampling(True), "s": lambda: s.r.set_sky(sky)}[c]()
        assert s.r.kernel_info(3)["variant"] == pt.VARIANT_MATERIALS_LIGHTS_SKY
        SC.assert_same_bits(s.frame(basis), want, f"order {''.join(order)}")
        s.close()


# ---- 4. sphere lights and the sun together -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_three_lamps_and_the_sun_equal_the_model(pt, oracle, gpu, rng):
    """The sun is light 3 of the list: under Philox its draws are words 2 and 3 of the block with counter word 3 = 2."""
    sph, basis = SC.courtyard_three_lamps(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    want, info = _model(oracle, ("three lamps", rng), SIZE, 4, sph, basis, SC.SUNS["small"], None, True, rng)
    _exercised(info, None, ("sun_sampled", "sun_lit", "sun_shadowed", "sun_below", "sampled", "lit", "self"), 4, f"three lamps and the sun {rng}")
    assert info["lights"] == [3, 4, 5] and min(info["lit_per_light"]) >= FLOOR, info["lit_per_light"]
    img, _ = pt.render_frame(SIZE, SIZE, 4, sph, basis, light_sampling=True, sky=pt.CLEAR_SKY, rng_mode=RNGS[rng])
    SC.assert_same_bits(img, want, f"three lamps and the sun {rng}")


# ---- 5. the frame interfaces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_row_tile_equals_the_models_rows(pt, oracle, gpu, rng):
    want, _ = _courtyard_model(oracle, 4, 5, rng, True, True, "low")
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    rows, rinfo = SM.render_frame(SIZE, SIZE, 4, sph, basis, MM.sincos_of(oracle), SC.SUNS["low"], SC.COURTYARD_SMALLPT, light_sampling=True, rng=rng,
                                  philox=oracle.philox, row_begin=8, row_end=16)
    assert rinfo["sun_lit"] >= FLOOR and rinfo["escaped_later"] >= FLOOR
    SC.assert_same_bits(rows, want[8:16], "the model's rows [8, 16)")  # both generators are keyed on the pixel's id
    tile, _ = pt.render_frame(SIZE, SIZE, 4, sph, basis, materials=SC.COURTYARD_SMALLPT, light_sampling=True, sky=SC.to_pt(pt, SC.SUNS["low"]),
                              rng_mode=RNGS[rng], row_begin=8, row_end=16)
    SC.assert_same_bits(tile, rows, f"rows [8, 16) of 24 {rng}")


def test_planar_layout_and_display_vertices_hold_the_same_frame(pt, oracle, gpu):
    want, info = _courtyard_model(oracle, 4, 5, "xorwow", True, True, "low")
    assert info["sun_lit"] >= FLOOR
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    s = _Session(pt, SIZE, 4, sph, layout=pt.LAYOUT_PLANAR, persist_rng=False)
    s.r.set_materials(SC.COURTYARD_SMALLPT)
    s.r.set_light_sampling(True)
    s.r.set_sky(SC.to_pt(pt, SC.SUNS["low"]))
    d_vtx = pt.DeviceBuffer(SIZE * SIZE * 3 * 4)
    s.r.set_display(d_vtx.ptr)
    s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    planar = s.d_out.download(np.float32, (14, SIZE, SIZE))
    vtx = d_vtx.download(np.float32, (SIZE, SIZE, 3))
    d_vtx.free()
    s.close()
    SC.assert_same_bits(np.ascontiguousarray(planar.transpose(1, 2, 0)), want, "planar layout")
    SC.assert_same_bits(vtx, pt.display_pack(want), "display vertices")


def test_persisted_xorwow_state_follows_the_model_over_two_frames(pt, oracle, gpu):
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    s = _Session(pt, SIZE, 1, sph)
    s.r.set_materials(SC.COURTYARD_SMALLPT)
    s.r.set_light_sampling(True)
    s.r.set_sky(pt.CLEAR_SKY)
    state = _xorwow_of(oracle.setup_random(SIZE, SIZE), SIZE, SIZE)
    sampled = 0
    for frame in range(2):
        want, info = SM.render_frame(SIZE, SIZE, 1, sph, basis, MM.sincos_of(oracle), SC.SUNS["small"], SC.COURTYARD_SMALLPT, light_sampling=True, state=state)
        sampled += info["sun_sampled"]
        SC.assert_same_bits(s.frame(basis), want, f"persisted state, frame {frame}")
        state = info["state"]
        assert np.array_equal(s.r.get_rng_state(), _words_of(state)), frame
    assert sampled >= FLOOR
    s.close()


def test_a_batch_without_light_sampling_is_the_loop_of_single_frames(pt, oracle, gpu):
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=SIZE, height=SIZE)
    s = _Session(pt, SIZE, 4, sph, rng_mode=RNGS["philox"])
    s.r.set_sky(SC.to_pt(pt, SC.SUNS["wide"]))
    d_two = pt.DeviceBuffer(2 * s.r.tile_floats * 4)
    s.r.enqueue_frames(d_two.ptr, s.r.tile_floats, s.d_scene.ptr, s.n, [basis, basis], [SC.EYE, SC.EYE])
    pt.check(pt.lib.pt_device_synchronize())
    two = d_two.download(np.float32, (2, SIZE, SIZE, 14))
    d_two.free()
    s.close()
    for frame in range(2):
        want, _ = _model(oracle, ("batch", frame), SIZE, 4, sph, basis, SC.SUNS["wide"], None, False, "philox", frame=frame)
        SC.assert_same_bits(two[frame], want, f"batch frame {frame}")


# ---- 6. many spheres ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_floor", [False, True])
def test_twelve_random_spheres_under_the_clear_sky_equal_the_model(pt, oracle, gpu, with_floor):
    """Twelve spheres: past PT_SCREEN_MAX_SPHERES the search, the sun's shadow ray's too, takes its many-sphere path.  The random
    spheres are small (radius 0.5 .. 3): alone they leave 10 to 20 hits in a 24 x 24 frame, so the case names the escapes; with the
    courtyard's floor under them (13 spheres) it names the sun's counters too."""
    sph = pt.scene_random(12, seed=2, with_walls=False)
    if with_floor:
        sph = np.concatenate([sph, SC.floor_only()])
    basis = pt.camera_basis(width=SIZE, height=SIZE)
    want, info = _model(oracle, ("random", with_floor), SIZE, 4, sph, basis, pt.CLEAR_SKY.as_dict(), None, True)
    named = ("escaped_primary", "escaped_later", "up", "sun_sampled", "sun_lit") if with_floor else ("escaped_primary", "up", "ground")
    _exercised(info, None, named, 4, f"twelve random spheres, floor={with_floor}")
    img, _ = pt.render_frame(SIZE, SIZE, 4, sph, basis, light_sampling=True, sky=pt.CLEAR_SKY)
    SC.assert_same_bits(img, want, f"twelve random spheres, floor={with_floor}")


# ---- 7. build facts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
@pytest.mark.parametrize("sampling", [False, True])
def test_sky_builds_report_their_variant_and_no_scratch(pt, gpu, sampling, rng):
    r = pt.Renderer(SIZE, SIZE, 4, rng_mode=RNGS[rng])
    r.set_sky(pt.CLEAR_SKY)
    if sampling:
        r.set_light_sampling(True)
    info = r.kernel_info(3)
    print(f"kernel_info sampling={sampling} {rng}: {info}")
    r.destroy()
    assert info["variant"] == (pt.VARIANT_MATERIALS_LIGHTS_SKY if sampling else pt.VARIANT_MATERIALS_SKY)
    assert info["scratch_bytes"] == 0 and info["max_spheres"] == 64


# ---- 8. refusals launch nothing ---------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_launch_nothing(pt, gpu):
    sph, basis = SC.courtyard(pt.scene_cornell()), pt.camera_basis(width=16, height=16)
    for opts, msg in ((dict(fast_math=True), r"pt_renderer_set_sky: a fast_math renderer has no sky"),
                      (dict(variant=6), r"pt_renderer_set_sky: the renderer has an explicit kernel variant \(6\)")):
        r = pt.Renderer(16, 16, 1, **opts)
        with pytest.raises(pt.PtError, match=msg) as e:
            r.set_sky(pt.CLEAR_SKY)
        assert e.value.code == -1
        r.set_sky(None)  # clearing what is not set is no error
        r.destroy()
    s = _Session(pt, 16, 1, sph)
    with pytest.raises(pt.PtError, match=r"pt_sky_check: sun_cos 1 "):  # a bad sky leaves the renderer as it was
        s.r.set_sky(pt.Sky((1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 1, 0), 1.0, (1, 1, 1)))
    assert s.r.kernel_info(3)["variant"] not in (pt.VARIANT_MATERIALS_SKY, pt.VARIANT_MATERIALS_LIGHTS_SKY)
    s.r.set_sky(pt.CLEAR_SKY)
    sentinel = np.full(16 * 16 * 14, 12345.0, dtype=np.float32)
    with pytest.raises(pt.PtError, match=r"pt_progressive_create: the renderer has a sky \(pt_renderer_set_sky\)"):
        pt.Progressive(s.r)
    s.r.set_light_sampling(True)
    d_two = pt.DeviceBuffer(2 * s.r.tile_floats * 4)
    d_two.upload(np.concatenate([sentinel, sentinel]))
    with pytest.raises(pt.PtError, match=r"pt_renderer_enqueue_frames: the renderer samples its lights directly"):
        s.r.enqueue_frames(d_two.ptr, s.r.tile_floats, s.d_scene.ptr, s.n, [basis, basis], [SC.EYE, SC.EYE])
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(d_two.download(np.float32, (2 * sentinel.size,)), np.concatenate([sentinel, sentinel]))
    d_two.free()
    s.r.set_light_sampling(False)
    s.r.set_sky(None)
    p = pt.Progressive(s.r)  # a session made without a sky refuses its passes under one
    s.r.set_sky(pt.CLEAR_SKY)
    s.d_out.upload(sentinel)
    with pytest.raises(pt.PtError, match=r"pt_progressive: the renderer has a sky"):
        p.render(1, s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(s.d_out.download(np.float32, sentinel.shape), sentinel)
    p.destroy()
    s.close()
    # without a table a scene above PT_MATERIALS_MAX_SPHERES is PT_ELIMIT, by name, and nothing is launched
    big = pt.scene_random(65, seed=5, with_walls=False)
    s = _Session(pt, 16, 1, big)
    s.r.set_sky(pt.CLEAR_SKY)
    s.d_out.upload(sentinel)
    with pytest.raises(pt.PtError, match=r"render: 65 spheres exceed the 64 spheres \(PT_MATERIALS_MAX_SPHERES\) the sky kernel stages") as e:
        s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    assert e.value.code == -5  # PT_ELIMIT
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(s.d_out.download(np.float32, sentinel.shape), sentinel)
    s.close()


# ---- 9. command line ---------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_librarys_frame(pt, gpu, tmp_path):
    from conftest import ROOT
    from test_parity_gpu import _read_feature_exr

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    out = str(tmp_path / "sky")
    res = subprocess.run([exe, "--sky", "clear", "--direct-light", "--size", "24", "-s", "4", "--nobitmap", "-o", out], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    img, _ = pt.render_frame(SIZE, SIZE, 4, light_sampling=True, sky=pt.CLEAR_SKY, basis=pt.camera_basis(width=SIZE, height=SIZE))
    names, planes = _read_feature_exr(out + ".exr")
    src = {"Color.R": 0, "Color.G": 1, "Color.B": 2, "Normal.X": 3, "Normal.Y": 4, "Normal.Z": 5, "Albedo.R": 6, "Albedo.G": 7, "Albedo.B": 8,
           "Depth.Z": 9, "ColorVar.Z": 10, "NormalVar.Z": 11, "AlbedoVar.Z": 12, "DepthVar.Z": 13}
    assert len(names) == 14
    for k, nm in enumerate(names):
        assert np.array_equal(planes[k].view(np.uint32), img[..., src[nm]].view(np.uint32)), nm
    # (the command line's scenes have walls: no ray leaves them, and what the sky changes is the sun's samples -- every shadow ray
    # ends on a wall -- and, under XORWOW, the stream that their draws move)
    plain, _ = pt.render_frame(SIZE, SIZE, 4, light_sampling=True, basis=pt.camera_basis(width=SIZE, height=SIZE))
    assert not np.array_equal(plain[..., :3], img[..., :3])
    # the file form of the same sky gives the same bytes
    path = tmp_path / "clear.txt"
    path.write_text("zenith 0.18 0.36 0.80\nhorizon 0.80 0.85 0.90\nground 0.25 0.25 0.25\nsun 0.4 0.8 0.45 0.999 400 380 340\n")
    res = subprocess.run([exe, "--sky", str(path), "--direct-light", "--size", "24", "-s", "4", "--nobitmap", "-o", out + "_file"], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert open(out + ".exr", "rb").read() == open(out + "_file.exr", "rb").read()
