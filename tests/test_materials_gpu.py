"""Sphere materials on the device (csrc/pt_materials.hip): every frame bit for bit, all 14 channels, against the oracle (all-diffuse
table: the anchor) and against tests/materials_model.py, the definition in NumPy float32 (EXACTNESS.md A.22).

The 24 x 24 model frames of the smallpt box are computed once per table and shared.  Counters first: a case compares bits only
after the model has shown that the arms in question were taken, so no case passes by comparing nothing.  At 1 spp and 5 bounces a
single 24 x 24 frame reflects off the inside of the glass ball only 12 or 13 times; the floor of 20 per arm is therefore held per
table over its cases (every case compares the same arms), and per case wherever a frame has 4 samples per pixel."""
import os
import subprocess

import numpy as np
import pytest

import materials_cases as MC
import materials_model as MM

pytestmark = pytest.mark.gpu

RNGS = {"xorwow": 0, "philox": 1}


def _model(oracle, size, spp, spheres, basis, materials, rng="xorwow", **kw):
    return MM.render_frame(size, size, spp, spheres, basis, MM.sincos_of(oracle), materials, rng=rng, philox=oracle.philox, **kw)


class _Session:
    """A renderer, its scene and its frame buffer."""

    def __init__(self, pt, size, spp, spheres, materials=None, rows=None, **opts):
        self.pt, self.size = pt, size
        if rows:
            opts.update(row_begin=rows[0], row_end=rows[1])
        self.r = pt.Renderer(size, size, spp, **opts)
        self.d_scene, self.n = pt.upload_scene(spheres)
        self.d_out = pt.DeviceBuffer(max(self.r.tile_floats * 4, 4))
        if materials is not None:
            self.r.set_materials(materials)

    def frame(self, basis, eye=MC.EYE):
        self.r.render(self.d_out.ptr, self.d_scene.ptr, self.n, basis, eye)
        return self.d_out.download(np.float32, (self.r.rows, self.size, 14))

    def close(self):
        self.d_out.free()
        self.d_scene.free()
        self.r.destroy()


# ---- 1. all-diffuse table against the oracle -------------------------------------------------------------------------------------
def test_all_diffuse_xorwow_persisted_and_fresh_equal_the_oracle(pt, oracle, gpu):
    size, spp = 32, 4
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=32, height=32)
    s = _Session(pt, size, spp, sph, [(MC.DIFFUSE, 0.0)] * 9)
    assert s.r.kernel_info(9)["variant"] == pt.VARIANT_MATERIALS
    st = oracle.setup_random(size, size)
    for frame in range(2):
        ref = oracle.render(size, size, spp, spheres=sph, basis=basis, rng_state=st)
        MC.assert_same_bits(s.frame(basis), ref, f"persisted state, frame {frame}")
        assert np.array_equal(s.r.get_rng_state(), st)
    s.close()
    s = _Session(pt, size, spp, sph, [(MC.DIFFUSE, 0.0)] * 9, persist_rng=False)
    ref = oracle.render(size, size, spp, spheres=sph, basis=basis)
    for frame in range(2):  # a fresh generator every frame: the same frame twice
        MC.assert_same_bits(s.frame(basis), ref, f"fresh state, frame {frame}")
    s.close()


def test_all_diffuse_philox_two_frames_equal_the_oracle(pt, oracle, gpu):
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=32, height=32)
    s = _Session(pt, 32, 4, sph, [(MC.DIFFUSE, 0.0)] * 9, rng_mode=pt.RNG_PHILOX, seed=0x1234567811)
    for frame in range(2):
        ref = oracle.render(32, 32, 4, spheres=sph, basis=basis, rng_mode=1, seed=0x1234567811, frame=frame)
        MC.assert_same_bits(s.frame(basis), ref, f"philox frame {frame}")
    s.close()


@pytest.mark.parametrize("rng", sorted(RNGS))
def test_all_diffuse_one_sample_equals_the_oracle(pt, oracle, gpu, rng):
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=32, height=32)
    img, _ = pt.render_frame(32, 32, 1, sph, basis, materials=[(MC.DIFFUSE, 0.0)] * 9, rng_mode=RNGS[rng])
    MC.assert_same_bits(img, oracle.render(32, 32, 1, spheres=sph, basis=basis, rng_mode=RNGS[rng]), f"1 spp {rng}")


@pytest.mark.parametrize("walls", [True, False])
def test_all_diffuse_twelve_random_spheres_equal_the_oracle(pt, oracle, gpu, walls):
    """Twelve spheres: past PT_SCREEN_MAX_SPHERES, the search takes its many-sphere path; without walls paths leave the scene."""
    sph, basis = pt.scene_random(12, seed=3, with_walls=walls), pt.camera_basis(width=32, height=32)
    img, _ = pt.render_frame(32, 32, 4, sph, basis, materials=[(MC.DIFFUSE, 0.0)] * 12, max_bounces=3)
    MC.assert_same_bits(img, oracle.render(32, 32, 4, spheres=sph, basis=basis, max_bounces=3), f"12 spheres, walls {walls}")


# ---- 2. smallpt's box against the model ------------------------------------------------------------------------------------------
BOX_CASES = [(spp, mb, rng) for spp in (4, 1) for mb in (5, 8) for rng in sorted(RNGS)]


@pytest.fixture(scope="module")
def box_models(oracle):
    """{glossy: {(spp, max_bounces, rng): (frame, info)}} at 24 x 24, computed once."""
    sph, basis = oracle.scene_cornell(), oracle.camera_basis(w=24, h=24)
    return {glossy: {(spp, mb, rng): _model(oracle, 24, spp, sph, basis, MC.smallpt(glossy), rng, max_bounces=mb) for spp, mb, rng in BOX_CASES}
            for glossy in (False, True)}


@pytest.mark.parametrize("spp,mb,rng", BOX_CASES)
@pytest.mark.parametrize("glossy", [False, True])
def test_smallpt_box_equals_the_model(pt, oracle, gpu, box_models, glossy, spp, mb, rng):
    taken = ("diffuse", "glossy" if glossy else "mirror", "glass_reflect_front", "glass_reflect_inside", "glass_refract_front", "glass_refract_inside")
    total = {a: sum(info[a] for _, info in box_models[glossy].values()) for a in taken}
    want, info = box_models[glossy][(spp, mb, rng)]
    print(f"glossy {glossy} {spp} spp {mb} bounces {rng}: arms {MC.arms(info)}, over the table's cases {total}")
    assert min(total.values()) >= 20 and all(info[a] > 0 for a in taken), (total, MC.arms(info))
    if spp == 4:
        assert min(info[a] for a in taken) >= 20, MC.arms(info)
    assert info["mirror" if glossy else "glossy"] == 0
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=24, height=24)
    assert np.array_equal(basis, oracle.camera_basis(w=24, h=24))
    img, _ = pt.render_frame(24, 24, spp, sph, basis, materials=MC.smallpt(glossy), max_bounces=mb, rng_mode=RNGS[rng])
    MC.assert_same_bits(img, want, f"smallpt box glossy={glossy} {spp} spp {mb} bounces {rng}")


def test_smallpt_preset_is_the_table_of_the_cases(pt):
    assert [tuple(m) for m in pt.SMALLPT_MATERIALS] == MC.smallpt() and len(pt.scene_cornell()) == 9


# ---- 3. total internal reflection ------------------------------------------------------------------------------------------------
def test_total_internal_reflection_equals_the_model(pt, oracle, gpu):
    sph, basis = MC.inside_glass_furnace(), pt.camera_basis(width=24, height=24)
    table = [(MC.DIFFUSE, 0.0), (MC.GLASS, MC.INSIDE_ETA)]
    want, info = _model(oracle, 24, 4, sph, basis, table, max_bounces=8)
    print("inside the glass sphere:", MC.arms(info))
    assert info["tir"] >= 20 and info["glass_refract_inside"] >= 20, MC.arms(info)
    img, _ = pt.render_frame(24, 24, 4, sph, basis, materials=table, max_bounces=8)
    MC.assert_same_bits(img, want, "eye inside a glass sphere")


# ---- 4. ragged shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_ragged_frame_and_row_tile_equal_the_model(pt, oracle, gpu, rng):
    """33 x 33 = 1089 pixels: four full workgroups and a tail of 65 lanes, one full wave and one lane of the next."""
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=33, height=33)
    want, info = _model(oracle, 33, 2, sph, basis, MC.smallpt(), rng)
    assert info["mirror"] >= 20 and info["glass_refract_front"] >= 20
    img, _ = pt.render_frame(33, 33, 2, sph, basis, materials=MC.smallpt(), rng_mode=RNGS[rng])
    MC.assert_same_bits(img, want, f"33 x 33 {rng}")
    tile, _ = pt.render_frame(33, 33, 2, sph, basis, materials=MC.smallpt(), rng_mode=RNGS[rng], row_begin=5, row_end=21)
    MC.assert_same_bits(tile, img[5:21], f"rows [5, 21) of 33 x 33 {rng}")
    rows, _ = _model(oracle, 33, 2, sph, basis, MC.smallpt(), rng, row_begin=5, row_end=21)
    MC.assert_same_bits(rows, want[5:21], f"the model's rows [5, 21) {rng}")


def test_planar_layout_and_display_vertices_hold_the_same_frame(pt, gpu):
    """Both are supported, not refused: the planar frame is the interleaved one transposed, the vertices are pt_display_pack's."""
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=33, height=33)
    img, _ = pt.render_frame(33, 33, 2, sph, basis, materials=MC.smallpt())
    s = _Session(pt, 33, 2, sph, MC.smallpt(), layout=pt.LAYOUT_PLANAR)
    d_vtx = pt.DeviceBuffer(33 * 33 * 3 * 4)
    s.r.set_display(d_vtx.ptr)
    s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    planar = s.d_out.download(np.float32, (14, 33, 33))
    vtx = d_vtx.download(np.float32, (33, 33, 3))
    d_vtx.free()
    s.close()
    MC.assert_same_bits(np.ascontiguousarray(planar.transpose(1, 2, 0)), img, "planar layout")
    MC.assert_same_bits(vtx, pt.display_pack(img), "display vertices")


# ---- 5. mirror furnace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", sorted(RNGS))
def test_mirror_furnace_is_exactly_the_emission(pt, gpu, rng):
    sph, basis = MC.ball_furnace(), pt.camera_basis(width=24, height=24)
    img, _ = pt.render_frame(24, 24, 4, sph, basis, materials=[(MC.DIFFUSE, 0.0), (MC.MIRROR, 0.0)], max_bounces=3, rng_mode=RNGS[rng])
    on_ball = img[..., 6] == 1.0  # the albedo of every sample is the ball's
    assert 20 <= np.count_nonzero(on_ball) < on_ball.size
    for k in range(3):
        assert np.all(img[..., k] == np.float32(MC.E[k])), k
    assert np.all(img[..., 10] == 0.0)


# ---- 6. set and clear ---------------------------------------------------------------------------------------------------------------
def test_set_and_clear_return_to_the_oracle_frame(pt, oracle, gpu):
    size, spp = 32, 4
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=32, height=32)
    s = _Session(pt, size, spp, sph)
    plain = s.r.kernel_info(9)["variant"]
    assert plain != pt.VARIANT_MATERIALS
    st = oracle.setup_random(size, size)
    MC.assert_same_bits(s.frame(basis), oracle.render(size, size, spp, spheres=sph, basis=basis, rng_state=st), "before a table")
    s.r.set_materials(pt.SMALLPT_MATERIALS)
    info = s.r.kernel_info(9)
    assert info["variant"] == pt.VARIANT_MATERIALS and info["scratch_bytes"] == 0 and info["num_vgprs"] <= 128
    want, minfo = _model(oracle, size, spp, sph, basis, MC.smallpt(), state=_xorwow_of(st))
    MC.assert_same_bits(s.frame(basis), want, "with the table, from the persisted state")
    st = _words_of(minfo["state"])
    assert np.array_equal(s.r.get_rng_state(), st)
    s.r.set_materials(None)
    assert s.r.kernel_info(9)["variant"] == plain
    MC.assert_same_bits(s.frame(basis), oracle.render(size, size, spp, spheres=sph, basis=basis, rng_state=st), "after the clear")
    s.close()


def _xorwow_of(words):
    """The persisted generator state ([pixels][6] words: d, v0 .. v4) as the restatement's Xorwow over a square frame."""
    import numpy_restatement as NR

    n = int(round(len(words) ** 0.5))
    g = NR.Xorwow(np.zeros((n, n), dtype=np.uint64))
    g.d = words[:, 0].reshape(n, n).copy()
    g.v = [words[:, 1 + k].reshape(n, n).copy() for k in range(5)]
    return g


def _words_of(g):
    return np.stack([g.d.reshape(-1)] + [v.reshape(-1) for v in g.v], axis=1).astype(np.uint32)


# ---- 7. device-side refusals --------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(pt, gpu):
    sph, basis = pt.scene_cornell(), pt.camera_basis(width=16, height=16)
    s = _Session(pt, 16, 1, sph, [(MC.DIFFUSE, 0.0)] * 8)  # eight entries, nine spheres
    sentinel = np.full(16 * 16 * 14, 12345.0, dtype=np.float32)
    s.d_out.upload(sentinel)
    with pytest.raises(pt.PtError, match=r"n_spheres 9 differs from the 8 entries"):
        s.r.render(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    with pytest.raises(pt.PtError, match=r"n_spheres 9 differs from the 8 entries"):
        s.r.enqueue(s.d_out.ptr, s.d_scene.ptr, s.n, basis)
    pt.check(pt.lib.pt_device_synchronize())
    assert np.array_equal(s.d_out.download(np.float32, sentinel.shape), sentinel)
    with pytest.raises(pt.PtError, match=r"pt_progressive_create: the renderer has a material table"):
        pt.Progressive(s.r)
    with pytest.raises(pt.PtError, match=r"table\[1\]\.kind 7"):
        s.r.set_materials([(0, 0.0), (7, 0.0)])
    assert s.r.kernel_info(9)["variant"] == pt.VARIANT_MATERIALS  # a refused table leaves the one that was set
    s.close()
    for opts, msg in ((dict(fast_math=True), "fast_math renderer has no materials"), (dict(variant=6), "explicit kernel variant")):
        r = pt.Renderer(16, 16, 1, **opts)
        with pytest.raises(pt.PtError, match=msg):
            r.set_materials(pt.SMALLPT_MATERIALS)
        r.destroy()
    r = pt.Renderer(16, 16, 1)
    with pytest.raises(pt.PtError) as e:
        r.set_materials([(MC.DIFFUSE, 0.0)] * 65)
    assert e.value.code == -5  # PT_ELIMIT
    r.destroy()


def test_sixty_four_spheres_and_frame_batches_work(pt, oracle, gpu):
    sph, basis = pt.scene_random(64, seed=5, with_walls=True), pt.camera_basis(width=16, height=16)
    s = _Session(pt, 16, 2, sph, [(MC.DIFFUSE, 0.0)] * 64)
    st = oracle.setup_random(16, 16)
    MC.assert_same_bits(s.frame(basis), oracle.render(16, 16, 2, spheres=sph, basis=basis, rng_state=st), "64 spheres")
    # a batch of frames is the loop of single enqueues
    d_two = pt.DeviceBuffer(2 * s.r.tile_floats * 4)
    s.r.enqueue_frames(d_two.ptr, s.r.tile_floats, s.d_scene.ptr, s.n, [basis, basis], [MC.EYE, MC.EYE])
    pt.check(pt.lib.pt_device_synchronize())
    two = d_two.download(np.float32, (2, 16, 16, 14))
    d_two.free()
    for f in range(2):
        MC.assert_same_bits(two[f], oracle.render(16, 16, 2, spheres=sph, basis=basis, rng_state=st), f"batch frame {f}")
    s.close()


# ---- 8. command line ----------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_librarys_frame(pt, gpu, tmp_path):
    from conftest import ROOT
    from test_parity_gpu import _read_feature_exr

    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    out = str(tmp_path / "box")
    res = subprocess.run([exe, "--size", "32", "-s", "4", "--materials", "smallpt", "--nobitmap", "-o", out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    img, _ = pt.render_frame(32, 32, 4, materials=pt.SMALLPT_MATERIALS, basis=pt.camera_basis(width=32, height=32))
    names, planes = _read_feature_exr(out + ".exr")
    src = {"Color.R": 0, "Color.G": 1, "Color.B": 2, "Normal.X": 3, "Normal.Y": 4, "Normal.Z": 5, "Albedo.R": 6, "Albedo.G": 7, "Albedo.B": 8,
           "Depth.Z": 9, "ColorVar.Z": 10, "NormalVar.Z": 11, "AlbedoVar.Z": 12, "DepthVar.Z": 13}
    assert len(names) == 14
    for k, nm in enumerate(names):
        assert np.array_equal(planes[k].view(np.uint32), img[..., src[nm]].view(np.uint32)), nm
    plain, _ = pt.render_frame(32, 32, 4, basis=pt.camera_basis(width=32, height=32))
    assert not np.array_equal(plain[..., :3], img[..., :3])  # the balls are no longer diffuse
