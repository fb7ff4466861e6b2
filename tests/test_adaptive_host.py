"""CPU tests of adaptive sampling's host side: the CLI's --adaptive flags and their refusals (before any device is touched),
the C ABI's argument checks, and self-checks of the NumPy decision model the GPU tests compare the device with."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from adaptive_model import converged, dilate, luminance, next_active
from conftest import ROOT


def _pathtrace(args, tmp_path):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


def test_help_lists_adaptive(tmp_path):
    run = _pathtrace(["--help"], tmp_path)
    assert run.returncode == 0
    for flag in ("--adaptive", "--adaptive-min", "--adaptive-radius"):
        assert flag in run.stdout


@pytest.mark.parametrize("extra, names", [
    (["--adaptive", "0.1"], ["--adaptive", "--progressive"]),
    (["--adaptive-min", "4"], ["--adaptive-min", "--progressive"]),
    (["--progressive", "2", "--adaptive-radius", "1"], ["--adaptive-radius", "--adaptive"]),
    (["--progressive", "2", "--adaptive", "-0.5"], ["--adaptive"]),
    (["--progressive", "2", "--adaptive", "nan"], ["--adaptive"]),
    (["--progressive", "2", "--adaptive", "inf"], ["--adaptive"]),
    (["--progressive", "2", "--adaptive", "0.1", "--adaptive-min", "1"], ["--adaptive-min"]),
    (["--progressive", "2", "--adaptive", "0.1", "--adaptive-radius", "5"], ["--adaptive-radius"]),
    (["--progressive", "2", "--adaptive", "0.1", "--adaptive-radius", "-1"], ["--adaptive-radius"]),
    (["--progressive", "2", "--adaptive", "0.1", "--frames", "3"], ["--progressive", "--frames"]),
    (["--progressive", "2", "--adaptive", "0.1", "--gpus", "2"], ["--progressive", "--gpus"]),
    (["--progressive", "0", "--adaptive", "0.1"], ["--progressive"]),
    (["--progressive", "1", "-s", "1", "--adaptive", "0.1"], ["--progressive", "-s"]),
])
def test_cli_refusals(tmp_path, extra, names):
    out = str(tmp_path / "o")
    run = _pathtrace(["--size", "16", "-o", out] + extra, tmp_path)
    assert run.returncode != 0
    assert "ERROR" in run.stderr and all(n in run.stderr for n in names), run.stderr
    assert "GPUassert" not in run.stderr
    assert not os.path.exists(out + ".exr")


def test_null_arguments_are_einval(pt):
    n = ctypes.c_int64(0)
    assert pt.lib.pt_progressive_set_adaptive(None, None) == -1
    assert pt.lib.pt_progressive_active(None, ctypes.byref(n)) == -1
    assert pt.lib.pt_progressive_counts(None, None, None) == -1
    assert "NULL" in pt.lib.pt_last_error().decode()


def test_python_view_exists(pt, lab):
    for m in ("set_adaptive", "active", "counts", "refine"):
        assert callable(getattr(pt.Progressive, m))
    for name in ("pt_debug_progressive_record", "pt_debug_progressive_set_active"):
        assert hasattr(lab.lib, name) and not hasattr(pt.lib, name)


# ---- the decision model on hand-built frames ------------------------------------------------------------------------------

def _frame(rows, w, lum=0.5, var=0.0):
    f = np.zeros((rows, w, 14), np.float32)
    f[..., 0:3] = lum  # grey: luminance == lum up to rounding
    f[..., 10] = var
    return f


def test_luminance_matches_the_reference_literals():
    c = np.array([1.0], np.float32)
    assert luminance(c, c, c)[0] == np.float32(0.2126 + 0.7152 + 0.0722)


def test_rule_b_threshold_and_floor():
    n = 16
    f = _frame(1, 4)
    lum = np.float64(luminance(f[..., 0], f[..., 1], f[..., 2])[0, 0])
    tol = np.float32(0.1)
    edge = np.float32((np.float64(tol) ** 2 * n) * lum * lum)  # (rounded to float: at or just around the threshold)
    f[0, :, 10] = [0.0, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1)) * 2, 1e30]
    full = np.full((1, 4), n)
    conv = converged(f, full, full, n, tol, 1e-3)
    assert conv.tolist() == [[True, True, False, False]]
    # a dark pixel: the floor, not its luminance, sets the scale
    d = _frame(1, 1, lum=0.0, var=np.float32(0.01 * 0.01 * n * 0.25 * 0.25 * 0.99))
    assert converged(d, np.full((1, 1), n), np.full((1, 1), n), n, 0.01, 0.25)[0, 0]
    assert not converged(d, np.full((1, 1), n), np.full((1, 1), n), n, 0.01, 0.01)[0, 0]


def test_rule_needs_every_sample_scored_and_n1_zero_stops():
    n = 8
    f = _frame(1, 3, var=0.0)
    n0 = np.array([[n, n - 1, 0]])
    n1 = np.array([[n, n, 0]])
    # zero variance converges only where n0 == n; n1 == 0 converges regardless
    assert converged(f, n0, n1, n, 0.0, 1.0).tolist() == [[True, False, True]]


def test_dilation_is_clipped_to_the_tile():
    u = np.zeros((5, 6), bool)
    u[0, 0] = True
    d1 = dilate(u, 1)
    assert d1.sum() == 4 and d1[:2, :2].all()
    u2 = np.zeros((5, 6), bool)
    u2[4, 5] = True
    d2 = dilate(u2, 2)
    assert d2.sum() == 9 and d2[2:, 3:].all()
    assert (dilate(u, 0) == u).all()
    # a window never wraps from a row's end to the next row's start
    u3 = np.zeros((3, 6), bool)
    u3[1, 5] = True
    assert not dilate(u3, 1)[:, 0].any()


def test_next_active_is_monotone_and_waits_for_min_samples():
    rng = np.random.default_rng(3)
    rows, w, n = 7, 9, 16
    f = _frame(rows, w)
    f[..., 10] = rng.uniform(0, 0.02, (rows, w)).astype(np.float32)
    full = np.full((rows, w), n)
    active = rng.uniform(size=(rows, w)) < 0.7
    for radius in (0, 1, 2):
        nxt = next_active(active, f, full, full, n, 0.1, 0.05, 2, radius)
        assert not (nxt & ~active).any()
    assert (next_active(active, f, full, full, n, 10.0, 0.05, n + 1, 1) == active).all()
    assert not next_active(active, f, full, full, n, 10.0, 0.05, n, 1).any()


def test_nan_luminance_takes_the_floor_and_nan_variance_never_converges():
    """The header's max is C's lum > floor ? lum : floor: a NaN luminance compares false and takes the floor; a NaN variance
    compares false against any threshold (include/ptcore.h, EXACTNESS.md A.20)."""
    n = 8
    full = np.full((1, 4), n)
    f = _frame(1, 4)
    f[0, 0, 0:3] = np.nan                      # NaN colour, variance 0: converged at the floor's threshold
    f[0, 1, 1] = np.nan                        # one NaN channel is a NaN luminance too
    f[0, 1, 10] = np.float32(0.5 * 0.5 * n * 2.0 * 2.0)      # exactly T(floor = 2): converged
    f[0, 2, 0:3] = np.nan
    f[0, 2, 10] = np.nextafter(np.float32(0.5 * 0.5 * n * 2.0 * 2.0), np.float32(np.inf))  # one float above T(floor): not
    f[0, 3, 10] = np.nan                       # NaN variance: never, whatever the tolerance
    assert converged(f, full, full, n, 0.5, 2.0).tolist() == [[True, True, False, False]]
    assert not converged(f, full, full, n, 1e30, 2.0)[0, 3]
    # and the sets: the NaN-variance pixel stays active, the NaN-colour pixel with variance 0 stops
    nxt = next_active(np.ones((1, 4), bool), f, full, full, n, 0.5, 2.0, 2, 0)
    assert nxt.tolist() == [[False, False, True, True]]
