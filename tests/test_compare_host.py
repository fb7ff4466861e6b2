"""CPU tests of the comparison stage (pt_compare_*, DENOISER.md "Frame comparison"): the exported symbols, the window's weights, the
float32 NumPy model (tests/compare_model.py) against its float64 twin on random frames and on a rendered Cornell pair from the
oracle, the model's known answers, and every refusal that comes before the device check."""
import ctypes
import math
import os

import numpy as np
import pytest

import compare_model as cm
import compare_refusal_cases as crc
import filter_model as fm
from conftest import ROOT

F = np.float32
SYMBOLS = ["pt_compare_opts_default", "pt_compare_create", "pt_compare_destroy", "pt_compare_workspace_bytes", "pt_compare_reserve_frames",
           "pt_compare_ssim_weights", "pt_compare_enqueue", "pt_compare_run", "pt_compare_enqueue_frames", "pt_compare_run_frames",
           "pt_compare_result"]

# The largest differences between the float32 model and its float64 twin, measured by this file's own `twin_differences` on the
# frames of test_the_model_stays_near_its_float64_twin (DENOISER.md, "Frame comparison", quotes them): per pixel |m - m64|,
# |r - r64| / max(r64, 1), |s - s64|; per frame |mse - mse64|, |relmse - relmse64| / relmse64, |ssim - ssim64|.
RECORDED = {
    "random": dict(m=1.78e-7, r=3.64e-7, s=2.18e-6, mse=2.07e-10, relmse=8.0e-9, ssim=1.53e-8),
    "cornell": dict(m=2.74e-7, r=1.71e-7, s=6.25e-7, mse=2.69e-10, relmse=1.15e-8, ssim=2.52e-11),
}
MARGIN = 4.0


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_the_abi_version_stays(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.CompareOpts) == 16 and ctypes.sizeof(pt.CompareValues) == 88
    o = pt.CompareOpts(max_frames=9, reserved=(1, 2, 3))
    pt.lib.pt_compare_opts_default(ctypes.byref(o))
    assert o.max_frames == 1 and tuple(o.reserved) == (0, 0, 0)
    pt.lib.pt_compare_opts_default(None)  # (a no-op)
    assert pt.lib.pt_compare_destroy(None) == 0


def test_refusals_come_before_the_device(pt):
    cases = crc.host_cases(pt)
    assert crc.play(pt, cases) == len(cases) >= 20
    assert {entry for _, entry, _, _ in cases} | {"pt_compare_destroy", "pt_compare_opts_default"} >= crc.HOST_ENTRIES
    assert sum(cid.startswith("create.") for cid, _, _, _ in cases) >= 12


def test_a_valid_create_needs_a_device_and_nothing_else(pt):
    """With every argument valid the only refusal left is the device's: no CPU fallback."""
    h = ctypes.c_void_p(0xdead)
    rc = pt.lib.pt_compare_create(64, 64, None, ctypes.byref(h))
    msg = pt.lib.pt_last_error().decode()
    n = ctypes.c_int(0)
    if pt.lib.pt_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        assert rc == 0 and h.value and pt.lib.pt_compare_destroy(h) == 0
    else:
        assert rc == -3 and h.value is None and "pt_compare_create" in msg  # PT_ENODEVICE


# ---- the weights ----------------------------------------------------------------------------------------------------

def test_weights_equal_the_model_sum_to_one_and_are_symmetric(pt):
    w, want = pt.ssim_weights(), cm.weights()
    assert w.dtype == np.float32 and np.array_equal(cm.bits(w), cm.bits(want))
    assert np.array_equal(cm.bits(w), cm.bits(w[::-1])) and (w > 0).all() and w[5] == w.max()
    # the doubles sum to 1 within a few ulps; rounding each to float32 moves it by at most half an ulp of itself
    exact = math.fsum(float(v) for v in cm.weights64())
    assert abs(exact - 1.0) < 1e-15
    assert abs(math.fsum(float(v) for v in w) - exact) <= sum(float(np.spacing(v)) / 2 for v in w)
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    assert np.abs(w - g / g.sum()).max() < 1e-7


# ---- the float64 twin -----------------------------------------------------------------------------------------------

def twin_differences(img, ref):
    got, want = cm.compare(img, ref), cm.twin(img, ref)
    return dict(m=float(np.abs(got["m"] - want["m"]).max()), r=float((np.abs(got["r"] - want["r"]) / np.maximum(want["r"], 1.0)).max()),
                s=float(np.abs(got["s"] - want["s"]).max()), mse=abs(got["mse"] - want["mse"]),
                relmse=abs(got["relmse"] - want["relmse"]) / max(want["relmse"], 1e-300), ssim=abs(got["ssim"] - want["ssim"])), got


def quantisation_holds(res):
    """Step 5: each floor loses less than one unit, so sum q <= (the exact sum of the float32 terms) x scale < sum q + pixels."""
    for key, field, scale in (("m", "sum_mse", cm.QM), ("r", "sum_relmse", cm.QR)):
        exact = math.fsum(res[key].astype(np.float64).ravel().tolist())  # (correctly rounded)
        lost = exact - res[field] / scale
        assert -1e-12 * max(exact, 1.0) <= lost <= res["pixels"] / scale, (key, lost)
    lost = math.fsum(res["s"].astype(np.float64).ravel().tolist()) - res["sum_ssim"] / cm.QS
    assert -1e-12 * res["pixels"] <= lost <= res["pixels"] / cm.QS


def _worst(pairs):
    worst = dict.fromkeys(("m", "r", "s", "mse", "relmse", "ssim"), 0.0)
    for img, ref in pairs:
        d, res = twin_differences(img, ref)
        quantisation_holds(res)
        worst = {k: max(worst[k], d[k]) for k in worst}
    return worst


def _assert_recorded(worst, which):
    print(which, {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= MARGIN * RECORDED[which][k], f"{which}: {k} differs from the float64 twin by {v:.3g}, recorded {RECORDED[which][k]:.3g}"


def test_the_model_stays_near_its_float64_twin_on_random_frames():
    pairs = [cm.hdr_pair(w, h, seed) for (w, h) in ((37, 29), (64, 64), (128, 128)) for seed in range(6)]
    _assert_recorded(_worst(pairs), "random")


@pytest.fixture(scope="module")
def cornell_pair(oracle, pt):
    basis = pt.camera_basis(width=64, height=64)
    return tuple(oracle.render(64, 64, spp, spheres=pt.scene_cornell(), basis=basis) for spp in (2, 64))


def test_the_model_stays_near_its_float64_twin_on_a_rendered_pair(cornell_pair):
    noisy, clean = cornell_pair
    _assert_recorded(_worst([(noisy, clean)]), "cornell")
    res = cm.compare(noisy, clean)
    assert 0.01 < res["rms"] < 0.5 and 0.0 < res["ssim"] < 0.9 and res["nonfinite"] == 0  # a noisy picture of the same scene


# ---- known answers --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", cm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_images_give_zero_error_and_ssim_exactly_one(size):
    w, h = size
    img, _ = cm.hdr_pair(w, h, seed=w + h)
    res = cm.compare(img, img)
    assert res["sum_mse"] == 0 and res["sum_relmse"] == 0 and res["saturated"] == 0
    assert (cm.bits(res["s"]) == 0x3F800000).all() and res["sum_ssim"] == (w * h) << 32
    assert (res["mse"], res["rms"], res["psnr"], res["relmse"], res["ssim"]) == (0.0, 0.0, math.inf, 0.0, 1.0)


def test_constant_images_have_known_sums():
    w, h = 37, 29
    res = cm.compare(np.full((h, w, 3), 0.75, F), np.full((h, w, 3), 0.25, F))
    assert res["sum_mse"] == int(w * h * 0.75 * 2 ** 34) and res["mse"] == 0.25 and res["rms"] == 0.5
    res = cm.compare(np.full((h, w, 3), 4.0, F), np.zeros((h, w, 3), F))
    assert (res["r"] == F(3072.0)).all() and res["saturated"] == 3 * w * h and res["relmse"] == 1024.0
    assert res["sum_mse"] == int(w * h * 3 * 2 ** 34)  # (the display shows 1 against 0)


def test_rms_agrees_with_the_filter_models_clamped_rms():
    """On a grid of multiples of 2^-10 every float32 operation of step 2 is exact and m 2^34 is an integer: the two agree to the
    double roundings of the two means.  On any image they agree within the quantisation, 2^-34 per pixel of sum m, plus the
    float32 roundings of m: five of them (two differences' worth in d d, the product, two adds), each at most 2^-24 of m."""
    rng = np.random.default_rng(5)
    a, b = (rng.integers(-200, 1500, (29, 37, 3)).astype(F) / F(1024.0) for _ in range(2))
    res = cm.compare(a, b)
    assert abs(res["rms"] - fm.clamped_rms(a, b)) <= 1e-15
    a, b = (rng.uniform(-0.2, 1.5, (29, 37, 3)).astype(F) for _ in range(2))
    res = cm.compare(a, b)
    want = fm.clamped_rms(a, b)
    bound_mse = 2.0 ** -34 / 3.0 + 5 * 2.0 ** -24 * res["mse"]
    assert abs(res["mse"] - want * want) <= bound_mse
    assert abs(res["rms"] - want) <= bound_mse / (res["rms"] + want)
