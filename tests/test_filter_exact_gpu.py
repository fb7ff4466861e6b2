"""The feature-guided filter's kernels (csrc/pt_filter.hip) on the exact cases of tests/filter_exact_cases.py: the set-up bit
for bit against the float32 model, every stop closed alone and the variance output against integer expectations, chains of
unfused iterations (the ping-pong), steps that no tap survives, small sigmas, non-finite frames and a frame with sky.

Exact cases compare bits.  The others use test_filter_gpu.py's measure and bound, E = max |hip - m64| / (|m64| + 1e-3) <=
16 x E32 with E32 the float32 model's value (equality where E32 is 0), over the pixels that are finite in the model.  The state
{ill', var'} comes out through the lab library's pt_debug_filter_state (FeatureFilter.state), which runs unfused iterations."""
import contextlib

import numpy as np
import pytest

import filter_exact_cases as fx
import filter_model as fm
from filter_exact_cases import bits

pytestmark = pytest.mark.gpu

FACTOR = 16.0
KINDS = [(kind, size) for kind in fx.STOPS for size in fx.SIZES]
IDS = [f"{kind}-{w}x{h}" for kind, (w, h) in KINDS]


@contextlib.contextmanager
def on_device(lab, frame, counts=None, **opts):
    """(filter, d_frame, d_rgb, d_counts pointer or None) for a host frame, from the lab library."""
    h, w = frame.shape[:2]
    ff = lab.FeatureFilter(w, h, **opts)
    bufs = [lab.DeviceBuffer(frame.nbytes).upload(frame), lab.DeviceBuffer(h * w * 12)]
    if counts is not None:
        bufs.append(lab.DeviceBuffer(h * w * 4).upload(np.ascontiguousarray(counts, dtype=np.uint32)))
    try:
        yield ff, bufs[0], bufs[1], (bufs[2].ptr if counts is not None else None)
    finally:
        for b in bufs:
            b.free()
        ff.destroy()


def parity(got, m64, m32, what):
    """The suite's bound over the pixels finite in the float64 model; prints and returns E / E32."""
    ok = np.isfinite(m64).all(-1)
    if not ok.any():
        return 0.0
    assert np.isfinite(np.asarray(got)[ok]).all(), what
    e, e32 = fm.rel_err(np.asarray(got)[ok], m64[ok]), fm.rel_err(m32[ok], m64[ok])
    print(f"PARITY {what}: E = {e:.3e}, E32 = {e32:.3e}, E / E32 = {e / e32 if e32 else float('nan'):.2f}")
    assert e <= FACTOR * e32, (what, e, e32)
    return e / e32 if e32 else 0.0


def model_pair(frame, **args):
    return fm.filter_model(frame, dtype=np.float64, **args), fm.filter_model(frame, dtype=np.float32, **args)


def check_steps(lab, c, steps, **sigmas):
    """Every step singly, through the tile and through direct loads: the fused iteration's colour and the unfused iteration's
    state {ill', var'} are the integer expectation's bits (and so the model's: test_filter_exact_host.py)."""
    frame = c["frame"]
    h, w = frame.shape[:2]
    with on_device(lab, frame, **{**c["sigmas"], **sigmas}) as (ff, d_frame, d_rgb, _):
        for step in steps:
            ill, var = fx.expected_step(c, step)[:2]
            rgb = ill * c["a"][..., None]  # (a power of two: exact)
            for tiled in (True, False):
                ff.tiled(tiled)
                ff.step(d_frame.ptr, fx.N, step, d_rgb=d_rgb.ptr)
                got = d_rgb.download(np.float32, (h, w, 3))
                assert np.array_equal(bits(got), bits(rgb)), (step, tiled, np.argwhere(bits(got) != bits(rgb))[:5])
                state, _, _ = ff.state(d_frame.ptr, fx.N, [step])
                assert np.array_equal(bits(state[..., :3]), bits(ill)), (step, tiled, np.argwhere(bits(state[..., :3]) != bits(ill))[:5])
                assert np.array_equal(bits(state[..., 3]), bits(var)), (step, tiled, np.argwhere(bits(state[..., 3]) != bits(var))[:5])
        assert d_frame.download(np.float32, frame.shape).tobytes() == frame.tobytes()  # the export only reads the frame


# ---- the set-up ---------------------------------------------------------------------------------------------------------

def check_setup(lab, name, frame, samples, counts):
    h, w = frame.shape[:2]
    ill, var, dz, _ = fm.setup(frame, samples=samples, counts=counts, dtype=np.float32)
    n_z, alb = fx.guides_of(frame)
    with on_device(lab, frame, counts) as (ff, d_frame, _, d_counts):
        state, g0, g1 = ff.state(d_frame.ptr, samples, (), d_counts=d_counts)
    for what, got, want in (("ill", state[..., :3], ill), ("var", state[..., 3], var), ("n, z", g0, n_z), ("albedo", g1[..., :3], alb),
                            ("dz", g1[..., 3], dz)):
        diff = bits(got) != bits(want)
        assert not diff.any(), (name, what, int(diff.sum()), np.argwhere(diff)[:5])


@pytest.mark.parametrize("k", range(len(fx.setup_inputs())), ids=[i[0].replace(" ", "-") for i in fx.setup_inputs()])
def test_the_set_up_gives_the_float32_models_bits(lab, gpu, k):
    """The state after 0 iterations and both guides, bit for bit fm.setup() in float32: prepare_kernel rounds operation by
    operation (test_filter_exact_host.py shows that two rounding-level mutants change bits on these inputs)."""
    check_setup(lab, *fx.setup_inputs()[k])


_sky = {}


def sky_frame(pt):
    """48 x 40, 4 spp of scene_random(40, with_walls=False) with every fifth sphere a light (the scene itself has none: every
    colour would be 0), rendered on the device from a camera that sees sky and spheres."""
    if not _sky:
        w, h, spp = 48, 40, 4
        eye = (50.0, 25.0, 110.0)
        spheres = pt.scene_random(40, with_walls=False)
        spheres["emission"][::5] = 12.0
        frame, _ = pt.render_frame(w, h, spp, spheres=spheres, basis=pt.camera_basis(eye, width=w, height=h), eye=eye)
        frame.setflags(write=False)
        sky = (frame[..., 3:11] == 0).all(-1)  # normal, albedo, depth and channel 10 all 0
        assert sky.any() and (~sky).sum() >= 40 and (frame[sky][..., :3] == 0).all() and (frame[~sky][..., :3] > 0).any()
        _sky.update(frame=frame, spp=spp, sky=sky)
    return _sky["frame"], _sky["spp"], _sky["sky"]


def test_the_set_up_of_a_frame_with_sky(pt, lab, gpu):
    frame, spp, sky = sky_frame(pt)
    check_setup(lab, "sky", frame, spp, None)
    dz = fm.setup(frame, samples=spp, dtype=np.float32)[2]
    assert (dz[sky] > 0).any() and (dz[sky] == 0).any()  # sky beside a sphere, and sky beside sky


def test_a_frame_with_sky_stays_finite_and_its_sky_black(pt, lab, gpu):
    frame, spp, sky = sky_frame(pt)
    for it in range(1, 6):
        rgb = pt.filter_frame(frame, spp, iterations=it)[..., :3]
        assert np.isfinite(rgb).all() and (rgb[sky] == 0).all(), it
        parity(rgb, *model_pair(frame, samples=spp, iterations=it), f"sky 48x40 iterations {it}")


# ---- one stop at a time, the variance, chains -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,size", KINDS, ids=IDS)
def test_one_closed_stop_is_the_exact_mean_over_the_class(lab, gpu, kind, size):
    check_steps(lab, fx.case(kind, *size), fx.STEPS)


@pytest.mark.parametrize("size", fx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_open_stops_give_the_exact_variance(lab, gpu, size):
    """var' = sum w^2 var / (sum w)^2 after one unfused iteration at each step, borders included."""
    check_steps(lab, fx.case("open", *size), fx.STEPS)


@pytest.mark.parametrize("size", fx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("steps", [(1, 2), (1, 2, 4)], ids=["1-2", "1-2-4"])
def test_chains_of_unfused_steps(lab, gpu, steps, size):
    """The ping-pong: the state after two and three unfused iterations is the integer expectation's bits wherever every tap of
    every iteration lay inside the frame (ill always, var while its numerators fit a float32), and over the whole frame the
    re-modulated state holds the parity bound against the float64 model's chain."""
    w, h = size
    c = fx.case("chain", w, h)
    frame = c["frame"]
    ill, var, margin = fx.expected_chain(c, steps)
    inner = (slice(margin, h - margin), slice(margin, w - margin))
    models = []
    for dtype in (np.float64, np.float32):
        m_ill, m_var, dz, a = fm.setup(frame, samples=fx.N, dtype=dtype)
        for s in steps:
            m_ill, m_var = fm.iterate(m_ill, m_var, frame, dz, s, **fx.OPEN)
        models.append(m_ill * a)
    with on_device(lab, frame, **fx.OPEN) as (ff, d_frame, _, _):
        for tiled in (True, False):
            ff.tiled(tiled)
            state, _, _ = ff.state(d_frame.ptr, fx.N, steps)
            assert np.array_equal(bits(state[inner][..., :3]), bits(ill[inner])), tiled
            if var is not None:
                assert np.array_equal(bits(state[inner][..., 3]), bits(var[inner])), tiled
            parity(state[..., :3] * c["a"][..., None], *models, f"chain {steps} {w}x{h} tiled {tiled}")


# ---- steps that no tap survives ---------------------------------------------------------------------------------------------

def test_a_step_larger_than_the_frame_keeps_the_centre_tap_alone(lab, gpu):
    """One fused iteration at step 64 on the 29 x 37 crop (37 columns, 29 rows), default sigmas: only the centre tap is inside
    the frame, its exponent is 0, and the kernel gives the float32 model's bits."""
    frame, spp = fx.crop(1, "29x37")
    h, w = frame.shape[:2]
    want = fm.filter_model(frame, samples=spp, steps=[64], dtype=np.float32)
    with on_device(lab, frame) as (ff, d_frame, d_rgb, _):
        ff.step(d_frame.ptr, spp, 64, d_rgb=d_rgb.ptr)
        got = d_rgb.download(np.float32, (h, w, 3))
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def test_eight_iterations_on_16x16_end_in_three_centre_only_steps(lab, gpu):
    """iterations = 8 on 16 x 16: the steps 32, 64 and 128 keep the centre tap alone.  From the kernel's own state after the
    five steps that do have taps, the float32 model's three further iterations and re-modulation give the kernel's bits."""
    frame = np.ascontiguousarray(fx.golden(1)[0][:16, :16])
    spp = 4
    with on_device(lab, frame, iterations=8) as (ff, d_frame, d_rgb, _):
        state, _, g1 = ff.state(d_frame.ptr, spp, (1, 2, 4, 8, 16))
        ff.run(d_frame.ptr, spp, d_rgb.ptr)
        got = d_rgb.download(np.float32, (16, 16, 3))
    ill, var, dz = state[..., :3].copy(), state[..., 3].copy(), g1[..., 3].copy()
    assert np.array_equal(bits(dz), bits(fm.setup(frame, samples=spp, dtype=np.float32)[2]))
    for step in (32, 64, 128):
        ill, var = fm.iterate(ill, var, frame, dz, step)
    want = ill * (fm.EPS32 + frame[..., 6:9])
    assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    parity(got, *model_pair(frame, samples=spp, iterations=8), "16x16 iterations 8")


@pytest.mark.parametrize("it", [6, 7, 8])
def test_more_than_five_iterations_hold_the_parity_bound(pt, gpu, it):
    frame, spp = fx.crop(1, "29x37")
    rgb = pt.filter_frame(frame, spp, iterations=it)[..., :3]
    assert np.isfinite(rgb).all()
    parity(rgb, *model_pair(frame, samples=spp, iterations=it), f"29x37 iterations {it}")


# ---- a sigma whose inverse square overflows -----------------------------------------------------------------------------------

@pytest.mark.parametrize("tiny", [1e-20, 1e-30])
@pytest.mark.parametrize("kind,sigma", [("normal", "sigma_n"), ("albedo", "sigma_a")])
def test_a_sigma_whose_inverse_square_overflows_is_a_hard_stop(pt, lab, gpu, kind, sigma, tiny):
    """log2(e) / sigma^2 is clamped to the largest float: the hard-switch frames give the bits of their 2^-10 / 2^-20 results,
    all finite (check_steps compares with finite expectations), and a golden crop holds the parity bound."""
    check_steps(lab, fx.case(kind, 37, 29), fx.STEPS, **{sigma: tiny})
    frame, spp = fx.crop(1, "29x37")
    rgb = pt.filter_frame(frame, spp, **{sigma: tiny})[..., :3]
    assert np.isfinite(rgb).all()
    parity(rgb, *model_pair(frame, samples=spp, **{sigma: tiny}), f"29x37 {sigma} {tiny:g}")


# ---- non-finite frames ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", list(fx.POISONS))
@pytest.mark.parametrize("where", list(fx.POISON_AT))
def test_a_non_finite_pixel_reaches_the_same_pixels_in_tile_direct_and_model(lab, gpu, where, what):
    """NaN or +inf in one pixel's colour, or NaN in its channel 10: after 1, 2 and 5 iterations the non-finite pixels of the
    output are the same through the tile, through direct loads and in the model, and the finite ones hold the parity bound."""
    frame, spp = fx.poisoned(where, what)
    h, w = frame.shape[:2]
    for it in (1, 2, 5):
        m64, m32 = model_pair(frame, samples=spp, iterations=it)
        bad = ~np.isfinite(m64)
        assert np.array_equal(bad, ~np.isfinite(m32))
        assert bad.any() == (what != "nan-var")  # (channel 10 only reaches var, which no output reads back)
        with on_device(lab, frame, iterations=it) as (ff, d_frame, d_rgb, _):
            for tiled in (True, False):
                ff.tiled(tiled)
                ff.run(d_frame.ptr, spp, d_rgb.ptr)
                got = d_rgb.download(np.float32, (h, w, 3))
                diff = ~np.isfinite(got) != bad
                assert not diff.any(), (it, tiled, int(diff.sum()), np.argwhere(diff)[:5])
                parity(got, m64, m32, f"{what} {where} iterations {it} tiled {tiled}")


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_a_poisoned_edge_pixel_does_not_reach_a_pixel_without_a_tap_there(lab, gpu, what):
    """One iteration at step 2 with (y, 0) poisoned: (y, 1) has its taps at columns 1, 3 and 5 and the skipped ones read its own
    column, so it stays finite in both forms ((y, 2), with a tap at column 0, does not)."""
    frame, spp = fx.poisoned("left", what)
    y, _ = fx.POISON_AT["left"]
    h, w = frame.shape[:2]
    bad = ~np.isfinite(fm.filter_model(frame, samples=spp, steps=[2]))
    assert not bad[y, 1].any() and bad[y, 2].all() and not bad[:, 1].any()
    with on_device(lab, frame) as (ff, d_frame, d_rgb, _):
        for tiled in (True, False):
            ff.tiled(tiled)
            ff.step(d_frame.ptr, spp, 2, d_rgb=d_rgb.ptr)
            got = d_rgb.download(np.float32, (h, w, 3))
            assert np.isfinite(got[y, 1]).all(), tiled
            assert np.array_equal(~np.isfinite(got), bad), tiled


def test_state_arguments_are_checked(lab, gpu):
    frame = np.ascontiguousarray(fx.golden(1)[0][:16, :16])
    with on_device(lab, frame) as (ff, d_frame, d_rgb, _):
        for steps, word in (((1,) * 9, "n_steps"), ((0,), "steps[0]"), ((1, 4097), "steps[1]")):
            with pytest.raises(lab.PtError, match=word.replace("[", r"\[").replace("]", r"\]")):
                ff.state(d_frame.ptr, 4, steps)
        with pytest.raises(lab.PtError, match="samples"):
            ff.state(d_frame.ptr, 0, (1,))
        arr = (lab.ctypes.c_int * 1)(1)
        assert lab.lib.pt_debug_filter_state(ff.handle, d_frame.ptr, 4, None, arr, 1, None, d_rgb.ptr, d_rgb.ptr) == -1
        assert "d_state" in lab.lib.pt_last_error().decode()
