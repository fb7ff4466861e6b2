"""CPU tests of the feature filter's spatial variance estimate (pt_filter_set_spatial; DENOISER.md, "Spatial variance estimate"):
the NumPy model's quality on oracle frames, alone and behind the temporal model, its float32 twin, its properties (who
qualifies, flat regions, a normal edge), the C ABI's option checks without a device, the exported symbols, and the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import filter_spatial_model as fsm
import temporal_model as tm
from conftest import ROOT

PT_EINVAL = -1
SYMBOLS = ("pt_filter_spatial_opts_default", "pt_filter_spatial_check", "pt_filter_set_spatial")


# ---- the model's quality ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def converged(oracle):
    """128 x 128 Cornell box, default camera, 4096 spp with another seed than the noisy frames (seed 0)."""
    basis = oracle.camera_basis(w=128, h=128)
    return basis, oracle.render(128, 128, 4096, basis=basis, seed=12345)[..., :3]


@pytest.mark.parametrize("spp,bound", [(1, 0.85), (2, 0.85), (4, 0.92), (8, 1.0), (16, 1.0)])
def test_model_lowers_the_error_of_low_sample_frames(oracle, converged, spp, bound):
    """R = 2, below = all: the float64 model's clamped-colour RMS error against the 4096-spp frame, over the plain model's.
    Measured with this model: 0.724, 0.725, 0.832, 0.908 and 0.953 at 1, 2, 4, 8 and 16 spp (plain 0.1118, 0.0952, 0.0621,
    0.0419, 0.0303; with the estimate 0.0810, 0.0690, 0.0517, 0.0380, 0.0289)."""
    basis, ref = converged
    frame = oracle.render(128, 128, spp, basis=basis)
    plain = fm.clamped_rms(fm.filter_model(frame, samples=spp), ref)
    spatial = fm.clamped_rms(fsm.filter_model(frame, samples=spp, below=fsm.ALL, radius=2), ref)
    print(f"SPATIAL spp {spp}: plain {plain:.4f} spatial {spatial:.4f} ratio {spatial / plain:.3f}")
    assert spatial <= bound * plain


def test_model_behind_the_temporal_model(oracle):
    """96 x 96, 1 spp, fly_pose(0 .. 9) with the generator state carried, each frame against its own 4096-spp frame of seed
    12345; the filter gets the temporal model's count image and below = 16.  Frames 0 and 1 at most 0.85 x accumulate + plain
    filter, no frame above 1.01 x.  Measured with these models: 0.756, 0.772, 0.879, 0.932, 0.953, 0.973, 0.982, 0.975, 0.964
    and 0.989 on frames 0 .. 9 (plain 0.1165 falling to 0.0478)."""
    size, n = 96, 1
    state = oracle.setup_random(size, size)
    model = tm.TemporalModel(size, size)
    ratios = []
    for k in range(10):
        eye, yaw = tm.fly_pose(k)
        basis = oracle.camera_basis(eye, yaw=yaw, w=size, h=size)
        frame = oracle.render(size, size, n, basis=basis, eye=eye, rng_state=state)
        ref = oracle.render(size, size, 4096, basis=basis, eye=eye, seed=12345)[..., :3]
        acc, counts = model.accumulate(frame, n, basis, eye)
        plain = fm.clamped_rms(fm.filter_model(acc, counts=counts), ref)
        spatial = fm.clamped_rms(fsm.filter_model(acc, counts=counts, below=16, radius=2), ref)
        print(f"SPATIAL temporal frame {k}: plain {plain:.4f} spatial {spatial:.4f} ratio {spatial / plain:.3f}")
        ratios.append(spatial / plain)
    assert ratios[0] <= 0.85 and ratios[1] <= 0.85, ratios
    assert max(ratios) <= 1.01, ratios


def test_float32_twin_stays_close_to_the_yardstick(oracle):
    """The closeness test_filter_host.py demands of the plain filter, with the estimate on (R = 1, 2, 3, below = all)."""
    frame = oracle.render(64, 64, 4, basis=oracle.camera_basis(w=64, h=64))
    for radius in (1, 2, 3):
        m64 = fsm.filter_model(frame, samples=4, below=fsm.ALL, radius=radius)
        m32 = fsm.filter_model(frame, samples=4, below=fsm.ALL, radius=radius, dtype=np.float32)
        assert m32.dtype == np.float32
        e32 = fm.rel_err(m32, m64)
        print(f"SPATIAL R = {radius}: E32 = {e32:.3g}")
        assert 0 < e32 < 1e-5
        assert not np.array_equal(m64, fm.filter_model(frame, samples=4))


# ---- the model's properties -------------------------------------------------------------------------------------------

def test_a_pixel_with_enough_samples_keeps_its_variance_exactly(oracle):
    frame = oracle.render(32, 32, 2, basis=oracle.camera_basis(w=32, h=32))
    counts = np.random.default_rng(3).choice(np.array([3, 4, 5], dtype=np.uint32), (32, 32))
    for dtype in (np.float64, np.float32):
        ill, var, dz, _ = fm.setup(frame, counts=counts, dtype=dtype)
        new = fsm.spatial_var(ill, var, frame, dz, 4, 2, counts=counts)
        keep = counts >= 4
        assert keep.any() and (~keep).any()
        assert new[keep].tobytes() == var[keep].tobytes()
        assert (new[~keep] >= var[~keep]).all() and (new[~keep] > var[~keep]).any()
        # the uniform count decides for the whole frame; below = 0 and a count at the threshold change nothing
        assert fsm.spatial_var(ill, var, frame, dz, 4, 2, samples=4) is var
        assert fsm.spatial_var(ill, var, frame, dz, 0, 2, samples=1) is var
        assert not np.array_equal(fsm.spatial_var(ill, var, frame, dz, 4, 2, samples=3), var)


def _plane(h, w, levels, left_normal=(1.0, 0.0, 0.0), right_normal=(0.0, 1.0, 0.0)):
    """Two half-planes, equal albedo and depth; illumination levels[0] left and levels[1] right, channel 10 zero."""
    frame = np.zeros((h, w, 14), np.float32)
    alb = np.float32(0.5)
    a = fm.EPS32 + alb
    left = np.arange(w) < w // 2
    frame[:, left, 3:6], frame[:, ~left, 3:6] = left_normal, right_normal
    frame[..., 6:9] = alb
    frame[..., 9] = 100.0
    frame[:, left, 0:3], frame[:, ~left, 0:3] = np.float32(levels[0]) * a, np.float32(levels[1]) * a
    return frame, left


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_uniform_illumination_gives_no_variance(radius):
    """Every tap has the pixel's luminance: the moments are taken of L_q - L_p, all exactly 0, so v is exactly 0 in float64 and
    in float32 (the mean of the luminances themselves would be off by a rounding, and v by its square); a 1 x 1 frame too."""
    frame, _ = _plane(12, 16, (3.0, 3.0), right_normal=(1.0, 0.0, 0.0))
    for dtype in (np.float64, np.float32):
        ill, var, dz, _ = fm.setup(frame, samples=4, dtype=dtype)
        v, sw, _ = fsm.estimate(ill, frame, dz, radius)
        assert sw.max() == (2 * radius + 1) ** 2 and sw.min() == (radius + 1) ** 2  # all weights 1, corners clipped
        assert (v == 0).all()
        one = np.ascontiguousarray(frame[:1, :1])
        ill, var, dz, _ = fm.setup(one, samples=4, dtype=dtype)
        v, sw, _ = fsm.estimate(ill, one, dz, radius)
        assert v[0, 0] == 0 and sw[0, 0] == 1
        assert fsm.spatial_var(ill, var, one, dz, fsm.ALL, radius, samples=4).tobytes() == var.tobytes()


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_the_other_side_of_a_normal_edge_does_not_enter(radius):
    """Two half-planes with unit normals 90 degrees apart; left, luminance alternates 1, 3 by column (spread 1 in a full window's
    columns), right it is S + the same, S = 100.  A tap across the edge has weight eps = exp(-2 / 0.35^2), about 8e-8, beside
    same-side weights of 1, so it adds at most eps (S + 2)^2 to the sum of w (L - m)^2 and moves m and the sum of w by parts in
    1e7: each side's v is what that side alone gives to within 2 eps S^2 = 1.6e-3 (a factor 2 over the first-order term for the
    rest).  Without the stop the step enters at S^2 x 2 / 9 or more, a million times that: the twin below."""
    h, w, S = 10, 24, 100.0
    frame, left = _plane(h, w, (0.0, 0.0))
    a = fm.EPS32 + np.float32(0.5)
    col = np.where(np.arange(w) % 2 == 0, 1.0, 3.0) + np.where(left, 0.0, S)
    frame[..., 0:3] = (col[None, :, None] * a).astype(np.float32)
    ill, var, dz, _ = fm.setup(frame, samples=4)
    v = fsm.estimate(ill, frame, dz, radius)[0]
    bound = 2.0 * np.exp(-2.0 / 0.35 ** 2) * S * S
    for side in (left, ~left):
        alone = np.ascontiguousarray(frame[:, side])
        ill_s, _, dz_s, _ = fm.setup(alone, samples=4)
        v_alone = fsm.estimate(ill_s, alone, dz_s, radius)[0]
        assert v_alone.min() > 0.5
        leak = float(np.abs(v[:, side] - v_alone).max())
        print(f"SPATIAL edge R = {radius}: leak {leak:.3e}, bound {bound:.3e}")
        assert leak <= bound, radius
    # without the edge the same frame's step enters the pixels beside it (the test above is not vacuous)
    frame[..., 3:6] = (1.0, 0.0, 0.0)
    ill, var, dz, _ = fm.setup(frame, samples=4)
    flat = fsm.estimate(ill, frame, dz, radius)[0]
    assert flat[:, w // 2 - 1].min() > 1e3 and flat[:, w // 2].min() > 1e3


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert "PT_FILTER_SPATIAL_ALL 0xFFFFFFFFu" in header and pt.FILTER_SPATIAL_ALL == 0xFFFFFFFF == fsm.ALL
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.FilterSpatialOpts) == 16 and ctypes.sizeof(pt.FilterOpts) == 32


def test_default_options(pt):
    o = pt.FilterSpatialOpts(below=7, radius=9)
    o.reserved[0] = o.reserved[1] = 5
    pt.lib.pt_filter_spatial_opts_default(ctypes.byref(o))
    assert (o.below, o.radius, tuple(o.reserved)) == (0, 2, (0, 0))
    pt.lib.pt_filter_spatial_opts_default(None)  # (a null pointer is ignored)
    assert pt.lib.pt_filter_spatial_check(ctypes.byref(o)) == 0


BAD = [(dict(radius=0), "radius 0"), (dict(radius=4), "radius 4"), (dict(radius=-1), "radius -1"), (dict(below=0, radius=7), "radius 7"),
       (dict(reserved=(1, 0)), "reserved[0]"), (dict(reserved=(0, -2)), "reserved[1]")]


@pytest.mark.parametrize("changes,word", BAD, ids=[w.replace(" ", "=") for _, w in BAD])
def test_check_and_set_refuse_every_bad_option_without_a_device(pt, changes, word):
    """PT_EINVAL naming the field from pt_filter_spatial_check, and from pt_filter_set_spatial, which checks the options before
    it looks at the filter (a null one here: there may be no device to make one on)."""
    args = dict(below=4, radius=2, reserved=(0, 0))
    args.update(changes)
    o = pt.FilterSpatialOpts(below=args["below"], radius=args["radius"])
    o.reserved[0], o.reserved[1] = args["reserved"]
    assert pt.lib.pt_filter_spatial_check(ctypes.byref(o)) == PT_EINVAL
    msg = pt.lib.pt_last_error().decode()
    assert word in msg and "pt_filter_spatial_check" in msg, msg
    with pytest.raises(pt.PtError, match="pt_filter_spatial_check"):
        pt.filter_spatial_check(args["below"], args["radius"], args["reserved"])
    assert pt.lib.pt_filter_set_spatial(None, ctypes.byref(o)) == PT_EINVAL  # (the options come before the filter)
    msg = pt.lib.pt_last_error().decode()
    assert word in msg and "pt_filter_set_spatial" in msg, msg
    if args["below"] and "reserved" not in changes:
        with pytest.raises(pt.PtError, match="pt_filter_spatial_check"):  # the constructor checks before it creates
            pt.FeatureFilter(16, 16, spatial_below=args["below"], spatial_radius=args["radius"])


def test_null_arguments_and_good_options(pt):
    assert pt.lib.pt_filter_spatial_check(None) == PT_EINVAL and "null opts" in pt.lib.pt_last_error().decode()
    o = pt.FilterSpatialOpts(below=4, radius=2)
    assert pt.lib.pt_filter_set_spatial(None, ctypes.byref(o)) == PT_EINVAL and "null filter" in pt.lib.pt_last_error().decode()
    assert pt.lib.pt_filter_set_spatial(None, None) == PT_EINVAL and "null filter" in pt.lib.pt_last_error().decode()
    for below in (0, 1, 16, 0xFFFFFFFF, "all"):
        for radius in (1, 2, 3):
            pt.filter_spatial_check(below, radius)
    with pytest.raises(ValueError):
        pt.filter_spatial_check(-1)
    with pytest.raises(ValueError):
        pt.filter_spatial_check(2 ** 32)


# ---- the CLI ------------------------------------------------------------------------------------------------------------

def _cli(tmp_path, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


@pytest.mark.parametrize("args,words", [
    (["--filter-spatial-below", "4"], ["--filter-spatial-below needs --filter"]),
    (["--filter", "--filter-spatial-radius", "2"], ["--filter-spatial-radius needs --filter-spatial-below"]),
    (["--filter", "--filter-spatial-below", "0"], ["--filter-spatial-below '0'", "or all"]),
    (["--filter", "--filter-spatial-below", "-3"], ["--filter-spatial-below '-3'", "or all"]),
    (["--filter", "--filter-spatial-below", "4x"], ["--filter-spatial-below '4x'", "or all"]),
    (["--filter", "--filter-spatial-below", "4294967296"], ["--filter-spatial-below '4294967296'"]),
    (["--filter", "--filter-spatial-below", "all", "--filter-spatial-radius", "0"], ["--filter-spatial-radius", "radius 0 outside 1 .. 3"]),
    (["--filter", "--filter-spatial-below", "4", "--filter-spatial-radius", "4"], ["--filter-spatial-radius", "radius 4 outside 1 .. 3"]),
], ids=["below-alone", "radius-alone", "below-0", "below-negative", "below-text", "below-2^32", "radius-0", "radius-4"])
def test_cli_refusals_come_before_any_device(tmp_path, args, words):
    """The device here would fail with a GPUassert line: none of these gets that far."""
    run = _cli(tmp_path, ["--size", "16", "--device", "99"] + args)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


def test_cli_help_lists_the_options(tmp_path):
    run = _cli(tmp_path, ["--help"])
    assert run.returncode == 0
    for opt in ("--filter-spatial-below", "--filter-spatial-radius"):
        assert opt in run.stdout
