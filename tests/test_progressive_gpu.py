"""Progressive sessions (pt_progressive_*, pixel_kernel's resume builds): a still frame refined pass by pass.  Contract
(include/ptcore.h, EXACTNESS.md A.19): after a pass that leaves the session at n >= 2 samples, the frame is bit for bit the first
Render() of a fresh renderer at n spp -- oracle.render(w, h, n, ..., frame=0) -- whatever the split of n into passes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_parity_gpu import assert_bit_exact

pytestmark = pytest.mark.gpu

EINVAL = -1
_oracle_cache = {}


def ref_frame(oracle, w, h, n, spheres, basis, mb, rng, row_begin=0, row_end=None, key=None):
    k = (key, w, h, n, mb, rng, row_begin, row_end)
    if key is None or k not in _oracle_cache:
        img = oracle.render(w, h, n, spheres=spheres, basis=basis, max_bounces=mb, rng_mode=rng, row_begin=row_begin,
                            row_end=row_end, frame=0, native=True)
        if key is None:
            return img
        _oracle_cache[k] = img
    return _oracle_cache[k]


def passes_against_oracle(pt, oracle, w, h, spheres, passes, mb, rng, key, variant=None, renderer_spp=None, **ropts):
    """Runs the passes, compares the frame after every pass that leaves n >= 2 with the oracle; returns the variants that ran."""
    basis = pt.camera_basis(width=w, height=h)
    r = pt.Renderer(w, h, renderer_spp or sum(passes), max_bounces=mb, rng_mode=rng, variant=variant, **ropts)
    s = pt.Progressive(r)
    d_scene, ns = pt.upload_scene(spheres)
    rows = r.rows
    d_out = pt.DeviceBuffer(rows * w * 56)
    ran = set()
    n = 0
    try:
        for p in passes:
            ran.add(s.variant(ns))
            s.render(p, d_out.ptr, d_scene.ptr, ns, basis)
            n += p
            assert s.samples() == n
            if n < 2:
                continue
            img = d_out.download(np.float32, (rows, w, 14))
            ref = ref_frame(oracle, w, h, n, spheres, basis, mb, rng, r.row_begin, r.row_end, key)
            assert_bit_exact(img, ref, f"{key} passes {passes} at n={n} rng {rng} bounces {mb} variant {variant}")
    finally:
        s.destroy()
        r.destroy()
        d_out.free()
        d_scene.free()
    return ran


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
@pytest.mark.parametrize("mb", [5, 8, 3])
@pytest.mark.parametrize("passes", [[3, 1, 4], [1, 1, 2]])
def test_reference_scene_against_oracle_after_every_pass(pt, oracle, gpu, rng, mb, passes):
    """96 x 64 (not a multiple of 64 wide): the REFB = 5 and 8 resume builds and the generic one (3 bounces)."""
    ran = passes_against_oracle(pt, oracle, 96, 64, pt.scene_cornell(), passes, mb, rng, key="cornell")
    assert ran == {6}


def _full_size(pt, w, h, spheres, mb, rng, passes, total):
    basis = pt.camera_basis(width=w, height=h)
    d_scene, ns = pt.upload_scene(spheres)
    d_a, d_b = pt.DeviceBuffer(w * h * 56), pt.DeviceBuffer(w * h * 56)
    r1 = pt.Renderer(w, h, total, max_bounces=mb, rng_mode=rng)
    r1.render(d_a.ptr, d_scene.ptr, ns, basis)
    r1.destroy()
    r2 = pt.Renderer(w, h, passes[0], max_bounces=mb, rng_mode=rng)
    s = pt.Progressive(r2)
    for p in passes:
        s.render(p, d_b.ptr, d_scene.ptr, ns, basis)
    v = s.variant(ns)
    s.destroy()
    r2.destroy()
    a, b = d_a.download(np.float32, (h, w, 14)), d_b.download(np.float32, (h, w, 14))
    for d in (d_a, d_b, d_scene):
        d.free()
    return a, b, v


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_headline_split_equals_one_render(pt, gpu, rng):
    """1024^2 x 5 bounces: 4 x 256 against the product's own 1024-spp Render() (chunked; pinned to the oracle elsewhere)."""
    a, b, v = _full_size(pt, 1024, 1024, pt.scene_cornell(), 5, rng, [256] * 4, 1024)
    assert v == 6
    assert_bit_exact(b, a, f"headline 4 x 256 vs 1024 rng {rng}")


def test_config4_split_equals_one_render(pt, gpu):
    """Config 4 (1000 random spheres, closed), 1024^2: 4 x 64 against 256."""
    a, b, v = _full_size(pt, 1024, 1024, pt.scene_random(1000, 1, True), 5, 0, [64] * 4, 256)
    assert v == 13
    assert_bit_exact(b, a, "config 4, 4 x 64 vs 256")


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_every_resume_variant_explicitly_and_automatically(pt, oracle, gpu, rng):
    """Random scenes of 40, 300 and 1300 spheres, open and closed, 64 x 48, passes [2, 5] against the oracle."""
    w, h, passes = 64, 48, [2, 5]
    ran = set()
    for n in (40, 300, 1300):
        for walls in (True, False):
            spheres = pt.scene_random(n, 7, walls)
            key = ("random", n, walls)
            explicit = [6, 10] + ([13] if n == 300 else []) + ([14] if n >= 300 else [])
            for v in explicit:
                assert passes_against_oracle(pt, oracle, w, h, spheres, passes, 5, rng, key, variant=v) == {v}
                ran.add(v)
            for rspp in (7, 16):  # (the automatic policy looks at the renderer's spp: 16 makes it pick 8 -> 6 for 40 spheres)
                got = passes_against_oracle(pt, oracle, w, h, spheres, passes, 5, rng, key, renderer_spp=rspp)
                assert len(got) == 1 and got <= {6, 10, 13, 14}
                ran |= got
    assert ran == {6, 10, 13, 14}


@pytest.mark.parametrize("v", [0, 8, 9])
def test_variants_without_resume_build_are_refused(pt, gpu, v):
    r = pt.Renderer(32, 32, 4, variant=v)
    with pytest.raises(pt.PtError) as e:
        pt.Progressive(r)
    assert e.value.code == EINVAL and str(v) in str(e.value)
    r.destroy()


def test_fast_math_renderer_is_refused(pt, gpu):
    r = pt.Renderer(32, 32, 4, fast_math=True)
    with pytest.raises(pt.PtError) as e:
        pt.Progressive(r)
    assert e.value.code == EINVAL and "fast_math" in str(e.value)
    r.destroy()


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_ragged_row_tile(pt, oracle, gpu, rng):
    """Rows 17..50 of 96 x 64: waves straddle rows, the last workgroup is partly empty."""
    passes_against_oracle(pt, oracle, 96, 64, pt.scene_cornell(), [3, 2, 3], 5, rng, key="tile", row_begin=17, row_end=50)


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_planar_layout(pt, oracle, gpu, rng):
    w, h, mb = 96, 64, 5
    basis = pt.camera_basis(width=w, height=h)
    r = pt.Renderer(w, h, 4, max_bounces=mb, rng_mode=rng, layout=pt.LAYOUT_PLANAR)
    s = pt.Progressive(r)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    d_out = pt.DeviceBuffer(w * h * 56)
    n = 0
    for p in (2, 3):
        s.render(p, d_out.ptr, d_scene.ptr, ns, basis)
        n += p
        planes = d_out.download(np.float32, (14, h, w))
        ref = ref_frame(oracle, w, h, n, pt.scene_cornell(), basis, mb, rng, key="cornell")
        assert_bit_exact(np.ascontiguousarray(planes.transpose(1, 2, 0)), ref, f"planar n={n}")
    s.destroy()
    r.destroy()


def test_render_calls_between_passes_do_not_interfere(pt, oracle, gpu):
    """Render() on the same renderer between passes: the session still matches the oracle, and the renderer's frames equal those
    of a twin renderer without a session (XORWOW, generator state persisted from frame to frame)."""
    w, h, mb = 96, 64, 5
    basis = pt.camera_basis(width=w, height=h)
    scene = pt.scene_cornell()
    r, twin = pt.Renderer(w, h, 4, max_bounces=mb), pt.Renderer(w, h, 4, max_bounces=mb)
    s = pt.Progressive(r)
    d_scene, ns = pt.upload_scene(scene)
    d_p, d_r, d_t = (pt.DeviceBuffer(w * h * 56) for _ in range(3))
    n = 0
    for p in (2, 3, 1):
        r.render(d_r.ptr, d_scene.ptr, ns, basis)
        twin.render(d_t.ptr, d_scene.ptr, ns, basis)
        assert_bit_exact(d_r.download(np.float32, (h, w, 14)), d_t.download(np.float32, (h, w, 14)), "renderer vs twin")
        s.render(p, d_p.ptr, d_scene.ptr, ns, basis)
        n += p
        ref = ref_frame(oracle, w, h, n, scene, basis, mb, 0, key="cornell")
        assert_bit_exact(d_p.download(np.float32, (h, w, 14)), ref, f"session at n={n} between Render() calls")
    assert np.array_equal(r.get_rng_state(), twin.get_rng_state())
    s.destroy()
    r.destroy()
    twin.destroy()


def test_d_out_is_output_only(pt, oracle, gpu):
    """Between passes: NaN in d_out, the denoiser in place on it, a different buffer.  Every next pass is still exact."""
    from cuda_pathtrace_amd import denoise_weights

    w, h, mb = 96, 64, 5
    basis = pt.camera_basis(width=w, height=h)
    scene = pt.scene_cornell()
    r = pt.Renderer(w, h, 4, max_bounces=mb)
    s = pt.Progressive(r)
    dn = pt.Denoiser(w, h, denoise_weights.random_state_dict(seed=1))
    d_scene, ns = pt.upload_scene(scene)
    d_a, d_b = pt.DeviceBuffer(w * h * 56), pt.DeviceBuffer(w * h * 56)
    nan = np.full((h, w, 14), np.nan, dtype=np.float32)
    n = 0
    for k, (p, buf) in enumerate([(2, d_a), (1, d_a), (3, d_a), (2, d_b), (2, d_a)]):
        s.render(p, buf.ptr, d_scene.ptr, ns, basis)
        n += p
        ref = ref_frame(oracle, w, h, n, scene, basis, mb, 0, key="cornell")
        assert_bit_exact(buf.download(np.float32, (h, w, 14)), ref, f"pass {k} at n={n}")
        if k == 0:
            buf.upload(nan)
        elif k == 1:
            dn.denoise(buf.ptr)  # in place: channels 0-2 and 9-13 rewritten
        elif k == 2:
            dn.denoise(buf.ptr)
    dn.destroy()
    s.destroy()
    r.destroy()


def test_reset_and_refusals(pt, lab, oracle, gpu):
    w, h, mb = 96, 64, 5
    basis = pt.camera_basis(width=w, height=h)
    scene = pt.scene_cornell()
    r = pt.Renderer(w, h, 4, max_bounces=mb)
    s = pt.Progressive(r)
    d_scene, ns = pt.upload_scene(scene)
    d_scene2, _ = pt.upload_scene(scene)
    d_out = pt.DeviceBuffer(w * h * 56)
    s.render(3, d_out.ptr, d_scene.ptr, ns, basis)
    other = np.array(basis, dtype=np.float32).copy()
    other[0] = np.nextafter(other[0], np.float32(np.inf))
    for args, what in [((2, d_out.ptr, d_scene.ptr, ns, other), "camera"),
                       ((2, d_out.ptr, d_scene.ptr, ns, basis, (50.0, 52.0, 295.5)), "eye"),
                       ((2, d_out.ptr, d_scene.ptr, ns - 1, basis), "n_spheres"),
                       ((2, d_out.ptr, d_scene2.ptr, ns, basis), "d_spheres")]:
        with pytest.raises(pt.PtError) as e:
            s.render(*args)
        assert e.value.code == EINVAL and "reset the session" in str(e.value), what
    for bad in (0, -3):
        with pytest.raises(pt.PtError) as e:
            s.render(bad, d_out.ptr, d_scene.ptr, ns, basis)
        assert e.value.code == EINVAL
    assert s.samples() == 3
    # reset, then a pass (on the camera refused above): what a new session gives
    s.reset()
    assert s.samples() == 0
    s.render(2, d_out.ptr, d_scene.ptr, ns, other)
    s.render(2, d_out.ptr, d_scene.ptr, ns, other)
    fresh = pt.Progressive(r)
    d_new = pt.DeviceBuffer(w * h * 56)
    fresh.render(4, d_new.ptr, d_scene.ptr, ns, other)
    assert_bit_exact(d_out.download(np.float32, (h, w, 14)), d_new.download(np.float32, (h, w, 14)), "reset session vs new session")
    assert_bit_exact(d_new.download(np.float32, (h, w, 14)), ref_frame(oracle, w, h, 4, scene, other, mb, 0), "after reset vs oracle")
    fresh.destroy()
    s.destroy()
    r.destroy()
    # the INT_MAX limit, through the lab library's setter (never by rendering that many samples)
    lr = lab.Renderer(8, 8, 2)
    ls = lab.Progressive(lr)
    ld_scene, lns = lab.upload_scene(scene)
    ld_out = lab.DeviceBuffer(8 * 8 * 56)
    lb = lab.camera_basis(width=8, height=8)
    for start, spp in ((2**31 - 2, 2), (2**31 - 1, 1)):
        ls.set_samples(start)
        with pytest.raises(lab.PtError) as e:
            ls.render(spp, ld_out.ptr, ld_scene.ptr, lns, lb)
        assert e.value.code == EINVAL and "INT_MAX" in str(e.value)
        assert ls.samples() == start
    ls.reset()
    ls.render(2, ld_out.ptr, ld_scene.ptr, lns, lb)
    assert ls.samples() == 2
    ls.destroy()
    lr.destroy()


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_cli_progressive_equals_one_frame(gpu, tmp_path, rng):
    """pathtrace --size 64 -s 8 --progressive 4 writes the EXR of pathtrace --size 64 -s 32, byte for byte."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    outs = []
    for name, extra in (("prog", ["-s", "8", "--progressive", "4"]), ("one", ["-s", "32"])):
        out = str(tmp_path / f"{name}_{rng}")
        run = subprocess.run([exe, "--size", "64", "--rng", rng, "-o", out, "--nobitmap"] + extra, capture_output=True, text=True,
                             timeout=120)
        assert run.returncode == 0, run.stderr
        assert "Render completed in" in run.stdout
        outs.append(open(out + ".exr", "rb").read())
        if name == "prog":
            assert "Progressive: 4 passes of 8 spp (32 spp)" in run.stdout
    assert outs[0] == outs[1]
