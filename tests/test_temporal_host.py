"""CPU tests of the temporal accumulator (pt_temporal_*, DENOISER.md "Temporal accumulation"): the exported symbols, the C ABI's
option checks without a device, the host camera step against the model bit for bit, the NumPy model's quality on oracle frames
of a fly-through, its agreement with a single frame of all the samples under a static camera, and the CLI's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import temporal_model as tm
from conftest import ROOT

PT_EINVAL = -1
SYMBOLS = ("pt_temporal_opts_default", "pt_temporal_create", "pt_temporal_destroy", "pt_temporal_reset", "pt_temporal_workspace_bytes",
           "pt_temporal_camera", "pt_temporal_enqueue", "pt_temporal_run", "pt_temporal_enqueue_frames", "pt_temporal_run_frames")
EYE = (50.0, 52.0, 295.6)


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.TemporalOpts) == 24


def test_default_options(pt):
    o = pt.TemporalOpts(history_cap=-1.0, reserved=7)
    pt.lib.pt_temporal_opts_default(ctypes.byref(o))
    assert (o.history_cap, o.depth_tol, o.normal_tol, o.albedo_tol, o.min_weight, o.reserved) == (
        256.0, np.float32(0.02), np.float32(0.9), np.float32(0.01), 0.25, 0)
    assert tm.DEFAULTS == dict(history_cap=256.0, depth_tol=0.02, normal_tol=0.9, albedo_tol=0.01, min_weight=0.25)


def _create(pt, width=64, height=64, **changes):
    o = pt.TemporalOpts()
    pt.lib.pt_temporal_opts_default(ctypes.byref(o))
    for k, v in changes.items():
        setattr(o, k, v)
    h = ctypes.c_void_p(0xdead)
    rc = pt.lib.pt_temporal_create(width, height, ctypes.byref(o), ctypes.byref(h))
    return rc, h.value, pt.lib.pt_last_error().decode()


@pytest.mark.parametrize("changes,word", [
    (dict(history_cap=0.5), "history_cap"), (dict(history_cap=float("nan")), "history_cap"), (dict(history_cap=-3.0), "history_cap"),
    (dict(depth_tol=0.0), "depth_tol"), (dict(depth_tol=float("inf")), "depth_tol"), (dict(depth_tol=float("nan")), "depth_tol"),
    (dict(normal_tol=1.5), "normal_tol"), (dict(normal_tol=-1.01), "normal_tol"), (dict(normal_tol=float("nan")), "normal_tol"),
    (dict(albedo_tol=0.0), "albedo_tol"), (dict(albedo_tol=float("inf")), "albedo_tol"), (dict(albedo_tol=-1.0), "albedo_tol"),
    (dict(min_weight=0.0), "min_weight"), (dict(min_weight=1.5), "min_weight"), (dict(min_weight=float("nan")), "min_weight"),
    (dict(reserved=1), "reserved"),
    (dict(width=0), "width 0 outside"), (dict(height=-3), "height -3 outside"), (dict(width=16385), "width 16385 outside"),
    (dict(width=8192, height=8192), "frame size 8192 x 8192"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_create_validates_every_option_before_a_device_is_touched(pt, changes, word):
    """PT_EINVAL naming the argument -- on a machine without a GPU too, where a valid create is PT_ENODEVICE / PT_EHIP."""
    rc, handle, msg = _create(pt, **changes)
    assert rc == PT_EINVAL and handle is None, (rc, msg)
    assert word in msg and "pt_temporal_create" in msg, msg


def test_null_arguments_are_refused_without_a_device(pt):
    assert pt.lib.pt_temporal_create(64, 64, None, None) == PT_EINVAL
    for call, word in [
        (lambda: pt.lib.pt_temporal_reset(None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_enqueue(None, None, 4, None, None, None, None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_run(None, None, 4, None, None, None, None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_enqueue_frames(None, 2, None, 14, None, None, 4, None, None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_run_frames(None, 2, None, 14, None, None, 4, None, None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_workspace_bytes(None, None), "null accumulator"),
        (lambda: pt.lib.pt_temporal_camera(None, None), "null basis"),
    ]:
        assert call() == PT_EINVAL
        assert word in pt.lib.pt_last_error().decode()
    assert pt.lib.pt_temporal_destroy(None) == 0


# ---- the host step --------------------------------------------------------------------------------------------------

CAMERAS = [
    dict(pos=EYE, yaw=-90.0, pitch=0.0, width=64, height=64),
    dict(pos=(56.0, 52.0, 287.6), yaw=-87.2, pitch=0.0, width=128, height=128),
    dict(pos=(50.0, 60.0, 250.0), yaw=-90.0, pitch=-17.5, width=64, height=64),
    dict(pos=(20.0, 30.0, 200.0), yaw=-61.0, pitch=12.25, width=96, height=96),
    dict(pos=EYE, yaw=60.0, pitch=-3.0, width=37, height=29),
    dict(pos=(70.0, 40.0, 120.0), yaw=-135.0, pitch=40.0, width=64, height=3),
]


@pytest.mark.parametrize("cam", CAMERAS, ids=lambda c: f"yaw{c['yaw']}-pitch{c['pitch']}-{c['width']}x{c['height']}")
def test_camera_matrix_equals_the_model_bit_for_bit(pt, cam):
    basis = pt.camera_basis(**cam)
    got, want = pt.temporal_camera(basis), tm.camera_matrix(basis)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # and it IS the inverse: P d = (1, sy, v) for a primary direction d = B0 + sy (B1 - B0) + v (B2 - B0)
    B = basis.reshape(4, 3).astype(np.float64)
    d = B[0] + 0.3 * (B[1] - B[0]) + 0.6 * (B[2] - B[0])
    assert np.allclose(got.astype(np.float64) @ d, (1.0, 0.3, 0.6), atol=1e-5)


def test_camera_refuses_degenerate_and_non_parallelogram_bases(pt):
    good = pt.camera_basis(width=64, height=64)
    flat = good.copy()
    flat[3:6] = flat[0:3]  # B1 = B0: no width
    skew = good.copy()
    skew[9] += 0.01 * float(np.linalg.norm(good[0:3]))  # B3 off the parallelogram by 1e-2 |B0|
    nan = good.copy()
    nan[4] = np.nan
    for basis, word in ((np.zeros(12, np.float32), "determinant"), (flat, "determinant"), (nan, "determinant"), (skew, "parallelogram")):
        with pytest.raises(pt.PtError) as err:
            pt.temporal_camera(basis)
        assert err.value.code == PT_EINVAL and word in str(err.value) and "basis" in str(err.value), str(err.value)
        with pytest.raises(ValueError):
            tm.camera_matrix(basis)
    nearly = good.copy()
    nearly[9] += 1e-4 * float(np.linalg.norm(good[0:3]))  # within the tolerance
    assert np.array_equal(pt.temporal_camera(nearly), tm.camera_matrix(nearly))


# ---- the model on oracle frames ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fly_through_table(oracle):
    """128 x 128 Cornell box, 12 poses, 4 spp with the generator state carried from frame to frame, each frame against its own
    2048-spp reference (another seed): per frame (valid share, noisy, accumulated, filtered, accumulated + filtered) clamped-
    colour RMS errors."""
    size, n = 128, 4
    state = oracle.setup_random(size, size)
    model = tm.TemporalModel(size, size)
    rows = []
    for k in range(12):
        eye, yaw = tm.fly_pose(k)
        basis = oracle.camera_basis(eye, yaw=yaw, w=size, h=size)
        frame = oracle.render(size, size, n, basis=basis, eye=eye, rng_state=state)
        ref = oracle.render(size, size, 2048, basis=basis, eye=eye, seed=12345)[..., :3]
        acc, counts = model.accumulate(frame, n, basis, eye)
        rows.append((float((counts > n).mean()), fm.clamped_rms(frame[..., :3], ref), fm.clamped_rms(acc[..., :3], ref),
                     fm.clamped_rms(fm.filter_model(frame, samples=n), ref), fm.clamped_rms(fm.filter_model(acc, counts=counts), ref)))
    print("frame  valid  noisy   accumulated (ratio)  filtered  accumulated+filtered (ratio)")
    for k, (valid, noisy, acc, filt, both) in enumerate(rows):
        print(f"{k:5d}  {valid:.3f}  {noisy:.4f}  {acc:.4f} ({acc / noisy:.3f})       {filt:.4f}    {both:.4f} ({both / filt:.3f})")
    return rows


def test_model_accumulation_halves_the_error_from_frame_8_on(fly_through_table):
    """Measured with this model: 0.295 .. 0.306 x the noisy frame's error on frames 8 .. 11, 94-95 % of the pixels with history."""
    for k, (valid, noisy, acc, _, _) in enumerate(fly_through_table):
        if k >= 1:
            assert valid >= 0.9, k
        if k >= 8:
            assert acc <= 0.5 * noisy, (k, acc, noisy)


def test_model_accumulation_then_filter_beats_the_filter_alone_from_frame_3_on(fly_through_table):
    """Measured with this model: 0.56 .. 0.65 x the filter's error on frames 3 .. 11."""
    for k, (_, _, _, filt, both) in enumerate(fly_through_table):
        if k >= 3:
            assert both <= 0.8 * filt, (k, both, filt)


def test_model_static_camera_equals_one_frame_of_all_samples(oracle):
    """4 frames of 4 spp at 64 x 64 with one XORWOW state carried across them hold the 16 samples of one 16-spp frame: where the
    accumulator kept every frame (count 16) its colour and merged variance are that frame's.  Measured: share 0.848, colour
    3.0e-3 (absolute 4.5e-6), variance 4.3e-3."""
    size, n = 64, 4
    basis = oracle.camera_basis(w=size, h=size)
    state = oracle.setup_random(size, size)
    model = tm.TemporalModel(size, size)
    for _ in range(4):
        acc, counts = model.accumulate(oracle.render(size, size, n, basis=basis, rng_state=state), n, basis, EYE)
    tm.static_check(acc, counts, oracle.render(size, size, 16, basis=basis), "model on oracle frames")


def test_model_first_frame_and_reset_pass_through():
    rng = np.random.default_rng(3)
    frame = rng.random((5, 7, 14), dtype=np.float32)
    frame[..., 3:6] = (0.0, 0.0, 1.0)
    frame[..., 9] += 1.0
    basis = np.array([-1, -1, -2, 1, -1, -2, -1, 1, -2, 1, 1, -2], np.float32)
    model = tm.TemporalModel(7, 5)
    for _ in range(2):
        out, counts = model.accumulate(frame, 4, basis, (0, 0, 0))
        assert out.tobytes() == frame.tobytes() and (counts == 4).all()
        again, counts = model.accumulate(frame, 4, basis, (0, 0, 0))
        # the same frame again: every pixel finds itself, the mean stays and the two equal groups of 4 merge to 6/7 of the variance
        assert (counts == 8).all() and np.allclose(again[..., :3], frame[..., :3], rtol=1e-5)
        assert np.allclose(again[..., 10], frame[..., 10] * (6.0 / 7.0), rtol=1e-4)
        assert again[..., 3:10].tobytes() == frame[..., 3:10].tobytes() and again[..., 11:].tobytes() == frame[..., 11:].tobytes()
        model.reset()


# ---- the CLI --------------------------------------------------------------------------------------------------------

def _cli(tmp_path, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


CLI_REFUSALS = [
    (["--temporal", "--progressive", "2"], ["--temporal cannot be combined with --progressive"]),
    (["--temporal", "--batch", "--poses", "none.txt"], ["--temporal cannot be combined with --batch"]),
    (["--temporal"], ["--temporal needs --frames or --poses"]),
    (["--frames", "3", "--temporal-cap", "16"], ["--temporal-cap needs --temporal"]),
    (["--frames", "3", "--temporal", "--temporal-cap", "0.5"], ["--temporal-cap 0.5", ">= 1"]),
    (["--frames", "3", "--temporal", "--temporal-cap", "nan"], ["--temporal-cap", "finite"]),
    (["--poses", "none.txt", "--temporal", "--temporal-cap", "inf"], ["--temporal-cap", "finite"]),
]
CLI_REFUSAL_IDS = ["with-progressive", "with-batch", "no-frame-loop", "cap-alone", "cap-below-1", "cap-nan", "cap-inf"]


@pytest.mark.parametrize("args,words", CLI_REFUSALS, ids=CLI_REFUSAL_IDS)
def test_cli_refusals_come_before_any_device(tmp_path, args, words):
    """The device here would fail with a GPUassert line: none of these gets that far."""
    run = _cli(tmp_path, ["--size", "16", "--device", "99"] + args)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


def test_cli_help_lists_the_flags(tmp_path):
    run = _cli(tmp_path, ["--help"])
    assert run.returncode == 0
    for opt in ("--temporal ", "--temporal-cap"):
        assert opt in run.stdout
