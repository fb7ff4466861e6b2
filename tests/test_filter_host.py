"""CPU tests of the feature-guided filter (pt_filter_*, DENOISER.md "Feature-guided filter"): the NumPy model's quality on
oracle frames and its edge stop, the C ABI's option checks without a device, the exported symbols, and the CLI's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
from conftest import ROOT

PT_EINVAL = -1
SYMBOLS = ("pt_filter_opts_default", "pt_filter_create", "pt_filter_destroy", "pt_filter_reserve_frames", "pt_filter_workspace_bytes",
           "pt_filter_enqueue", "pt_filter_run", "pt_filter_enqueue_frames", "pt_filter_run_frames")


# ---- the model ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def converged(oracle):
    """128 x 128 Cornell box, default camera, 4096 spp with another seed than the noisy frames (seed 0)."""
    basis = oracle.camera_basis(w=128, h=128)
    return basis, oracle.render(128, 128, 4096, basis=basis, seed=12345)[..., :3]


@pytest.mark.parametrize("spp", [2, 4, 16])
def test_model_halves_the_error_of_low_sample_frames(oracle, converged, spp):
    """The float64 model's clamped-colour RMS error against the 4096-spp frame is at most 0.5 x the noisy frame's (measured
    with this model: 0.36, 0.28 and 0.25 at 2, 4 and 16 spp)."""
    basis, ref = converged
    frame = oracle.render(128, 128, spp, basis=basis)
    noisy = fm.clamped_rms(frame[..., :3], ref)
    filtered = fm.clamped_rms(fm.filter_model(frame, samples=spp), ref)
    print(f"spp {spp}: noisy {noisy:.4f} filtered {filtered:.4f} ratio {filtered / noisy:.3f}")
    assert filtered <= 0.5 * noisy


def test_float32_twin_stays_close_to_the_yardstick(oracle):
    """The filter is well conditioned: the float32 twin is within a few float32 roundings of the float64 model."""
    frame = oracle.render(64, 64, 4, basis=oracle.camera_basis(w=64, h=64))
    m64, m32 = fm.filter_model(frame, samples=4), fm.filter_model(frame, samples=4, dtype=np.float32)
    assert m32.dtype == np.float32
    e32 = fm.rel_err(m32, m64)
    print(f"E32 = {e32:.3g}")
    assert 0 < e32 < 1e-5


def test_model_stops_at_a_normal_edge():
    """Two half-planes with unit normals 90 degrees apart, equal albedo and depth, constant illumination 1 and 10, variance
    large: after 5 iterations no output has moved by more than 1e-4 relative towards the other side (the weight across the
    edge is exp(-2 / 0.35^2), about 8e-8)."""
    h, w, spp = 24, 48, 4
    frame = np.zeros((h, w, 14), np.float32)
    alb = np.float32(0.5)
    a = fm.EPS32 + alb
    left = np.arange(w) < w // 2
    frame[:, left, 3], frame[:, ~left, 4] = 1.0, 1.0
    frame[..., 6:9] = alb
    frame[..., 9] = 100.0
    frame[:, left, 0:3], frame[:, ~left, 0:3] = np.float32(1.0) * a, np.float32(10.0) * a
    frame[..., 10] = 1000.0  # a standard error far above the step between the two sides: only the normal stops the filter
    out = fm.filter_model(frame, samples=spp) / np.float64(a)
    assert np.abs(out[:, left] - 1.0).max() <= 1e-4 * 1.0
    assert np.abs(out[:, ~left] - 10.0).max() <= 1e-4 * 10.0
    # and without the normal edge the same frame IS smoothed across the step (the test above is not vacuous)
    frame[..., 3], frame[..., 4] = 1.0, 0.0
    flat = fm.filter_model(frame, samples=spp) / np.float64(a)
    assert flat[:, w // 2 - 1].min() > 2.0


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    lab_header = open(os.path.join(ROOT, "include", "ptcore_lab.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert "pt_debug_filter_step(" in lab_header and "pt_debug_filter_step" in lab.LAB_ABI and hasattr(lab.lib, "pt_debug_filter_step")
    assert not hasattr(pt.lib, "pt_debug_filter_step")
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.FilterOpts) == 32


def test_default_options(pt):
    o = pt.FilterOpts(iterations=77)
    pt.lib.pt_filter_opts_default(ctypes.byref(o))
    assert (o.iterations, o.max_frames, tuple(o.reserved)) == (5, 1, (0, 0))
    assert (o.sigma_l, o.sigma_n, o.sigma_a, o.sigma_z) == (4.0, np.float32(0.35), np.float32(0.1), 1.0)


def _create(pt, width=64, height=64, **changes):
    o = pt.FilterOpts()
    pt.lib.pt_filter_opts_default(ctypes.byref(o))
    for k, v in changes.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    h = ctypes.c_void_p(0xdead)
    rc = pt.lib.pt_filter_create(width, height, ctypes.byref(o), ctypes.byref(h))
    return rc, h.value, pt.lib.pt_last_error().decode()


@pytest.mark.parametrize("changes,word", [
    (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
    (dict(sigma_l=0.0), "sigma_l"), (dict(sigma_n=-1.0), "sigma_n"), (dict(sigma_a=float("nan")), "sigma_a"),
    (dict(sigma_z=float("inf")), "sigma_z"), (dict(sigma_l=float("nan")), "sigma_l"), (dict(sigma_z=0.0), "sigma_z"),
    (dict(max_frames=0), "max_frames"), (dict(reserved=0), "reserved[0]"), (dict(reserved=1), "reserved[1]"),
    (dict(width=0), "width 0 outside"), (dict(height=-3), "height -3 outside"), (dict(width=16385), "width 16385 outside"),
    (dict(width=8192, height=8192), "frame size 8192 x 8192"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_create_validates_every_option_before_a_device_is_touched(pt, changes, word):
    """PT_EINVAL naming the argument -- on a machine without a GPU too, where a valid create is PT_ENODEVICE / PT_EHIP."""
    rc, handle, msg = _create(pt, **changes)
    assert rc == PT_EINVAL and handle is None, (rc, msg)
    assert word in msg and "pt_filter_create" in msg, msg


def test_null_arguments_are_refused_without_a_device(pt):
    assert pt.lib.pt_filter_create(64, 64, None, None) == PT_EINVAL
    for call, word in [
        (lambda: pt.lib.pt_filter_reserve_frames(None, 2), "null filter"),
        (lambda: pt.lib.pt_filter_enqueue(None, None, None, 4, None, None), "null filter"),
        (lambda: pt.lib.pt_filter_run(None, None, None, 4, None, None), "null filter"),
        (lambda: pt.lib.pt_filter_enqueue_frames(None, 2, None, 14, None, 0, 4, None), "null filter"),
        (lambda: pt.lib.pt_filter_run_frames(None, 2, None, 14, None, 0, 4, None), "null filter"),
        (lambda: pt.lib.pt_filter_workspace_bytes(None, None), "null filter"),
    ]:
        assert call() == PT_EINVAL
        assert word in pt.lib.pt_last_error().decode()
    assert pt.lib.pt_filter_destroy(None) == 0


# ---- the CLI --------------------------------------------------------------------------------------------------------

def _cli(tmp_path, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


@pytest.mark.parametrize("args,words", [
    (["--filter", "-d", "--denoise-weights", "none.ptdn"], ["--filter cannot be combined with -d"]),
    (["--filter", "--batch", "--poses", "none.txt"], ["--filter cannot be combined with --batch"]),
    (["--filter-iterations", "3"], ["--filter-iterations needs --filter"]),
    (["--filter-sigma", "4,0.35,0.1,1"], ["--filter-sigma needs --filter"]),
    (["--filter", "--filter-iterations", "0"], ["--filter-iterations 0", "1 .. 8"]),
    (["--filter", "--filter-iterations", "9"], ["--filter-iterations 9", "1 .. 8"]),
    (["--filter", "--filter-sigma", "4,0.35,0.1"], ["--filter-sigma '4,0.35,0.1'", "l,n,a,z"]),
    (["--filter", "--filter-sigma", "4,0.35,0,1"], ["--filter-sigma", "> 0"]),
    (["--filter", "--filter-sigma", "4,nan,0.1,1"], ["--filter-sigma", "finite"]),
    (["--filter", "--filter-sigma", "4,0.35,0.1,1,2"], ["--filter-sigma", "four"]),
], ids=["with-d", "with-batch", "iterations-alone", "sigma-alone", "iterations-0", "iterations-9", "sigma-three", "sigma-zero",
        "sigma-nan", "sigma-five"])
def test_cli_refusals_come_before_any_device(tmp_path, args, words):
    """The device here would fail with a GPUassert line: none of these gets that far."""
    run = _cli(tmp_path, ["--size", "16", "--device", "99"] + args)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


def test_cli_d_without_weights_keeps_its_error_and_help_lists_the_filter(tmp_path):
    run = _cli(tmp_path, ["--size", "16", "-d"])
    assert run.returncode == 1 and "-d needs the network's weights" in run.stderr
    run = _cli(tmp_path, ["--help"])
    assert run.returncode == 0
    for opt in ("--filter ", "--filter-iterations", "--filter-sigma"):
        assert opt in run.stdout
