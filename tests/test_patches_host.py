"""CPU tests of the training-patch stage (pt_patches_*, DENOISER.md "Training patches"): the exported symbols, every refusal that
comes before the device check, the known answers of the float32 NumPy model (tests/patches_model.py), the model against the
reference's float64 measure within a bound written as a formula, the selection loop pick_patches, and the C++ wrapper
host/PatchSampler.h in a stand-alone program."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import denoise_restatement as dr
import patches_model as pm
import patches_refusal_cases as prc
from conftest import GOLDEN, ROOT

F = np.float32
SYMBOLS = ["pt_patches_opts_default", "pt_patches_create", "pt_patches_destroy", "pt_patches_workspace_bytes", "pt_patches_prepare",
           "pt_patches_score", "pt_patches_result", "pt_patches_gather", "pt_patches_run_prepare", "pt_patches_run_score",
           "pt_patches_run_gather"]

# The largest |score - twin| / bound seen by test_the_model_stays_within_the_bound_of_the_float64_measure, per group of frames
# (printed by the test; DENOISER.md, "Training patches", quotes them).  Recorded, not asserted: the assertion is ratio <= 1.
RECORDED_RATIO = {"random": 0.798, "oracle": 0.308}


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_the_abi_version_stays(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.PatchesOpts) == 16 and ctypes.sizeof(pt.PatchesValues) == 96
    assert [n for n, _ in pt.PatchesValues._fields_] == list(pm.FIELDS)
    o = pt.PatchesOpts(patch=9, max_patches=9, reserved=(1, 2))
    pt.lib.pt_patches_opts_default(ctypes.byref(o))
    assert (o.patch, o.max_patches, tuple(o.reserved)) == (64, 64, (0, 0))
    pt.lib.pt_patches_opts_default(None)  # (a no-op)
    assert pt.lib.pt_patches_destroy(None) == 0


def test_refusals_come_before_the_device(pt):
    cases = prc.host_cases(pt)
    played = prc.play(pt, cases)
    assert played >= 20
    assert {entry for _, entry, _, _ in cases if entry} | {"pt_patches_destroy", "pt_patches_opts_default"} >= prc.HOST_ENTRIES
    assert sum(cid.startswith("create.") for cid, _, _, _ in cases) >= 10


def test_a_valid_create_needs_a_device_and_nothing_else(pt):
    """With every argument valid the only refusal left is the device's: no CPU fallback."""
    h = ctypes.c_void_p(0xdead)
    rc = pt.lib.pt_patches_create(64, 64, None, ctypes.byref(h))
    msg = pt.lib.pt_last_error().decode()
    n = ctypes.c_int(0)
    if pt.lib.pt_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        assert rc == 0 and h.value and pt.lib.pt_patches_destroy(h) == 0
    else:
        assert rc == -3 and h.value is None and "pt_patches_create" in msg  # PT_ENODEVICE


# ---- known answers of the model -------------------------------------------------------------------------------------

def test_the_models_preprocessing_is_the_networks():
    """Step 2 of the model and denoise_restatement.preprocess, which pt_denoiser_* is held to: the same bits."""
    for w, h, seed in ((37, 29, 1), (64, 48, 2)):
        frame, _ = pm.frame_pair(w, h, seed)
        with np.errstate(all="ignore"):
            want = dr.preprocess(frame)
        assert np.array_equal(pm.bits(pm.preprocess(frame)), pm.bits(want))


def test_fmaxf_ignores_a_nan_among_the_features():
    frame, _ = pm.frame_pair(37, 29, 3, nan_features=True)
    assert np.isnan(frame[..., 9:14]).any(axis=(0, 1)).all()
    want = [F(0.00316 + float(np.nanmax(frame[..., k]))) for k in range(9, 14)]
    assert np.array_equal(pm.bits(pm.divisors(frame)), pm.bits(want)) and np.isfinite(pm.divisors(frame)).all()
    frame[..., 12] = np.nan  # nothing but NaNs: the maximum stays -inf
    assert pm.divisors(frame)[3] == -np.inf


def test_a_constant_frame_scores_exactly_zero():
    frame = np.empty((16, 16, 14), F)
    frame[...] = np.repeat(np.array([0.7, 0.3, 0.5, 120.0, 0.01], F), (3, 3, 3, 1, 4))  # (one value per population)
    for res in pm.scores(frame, [(0, 0), (3, 5)], 8):
        assert res["score"] == 0.0 and res["var_colour"] == 0.0 and res["var_normal"] == 0.0
        assert res["values"] == 192 and res["colour_s1"] > 0 and res["normal_s1"] > 0


@pytest.mark.parametrize("p", [2, 8, 14])
@pytest.mark.parametrize("ab", [(0.75, 0.25), (3.5, -1.25), (1.0, 0.0), (2.0 ** -20, 0.0)])
def test_a_dyadic_checkerboard_scores_a_quarter_of_the_squared_step(ab, p):
    """Half of the values a, half b, both multiples of 2^-20 and P even: the variance is (a - b)^2 / 4 with no rounding
    anywhere.  The colour's population cannot be negative: its b is clamped to 0 first."""
    a, b = F(ab[0]), F(ab[1])
    yy, xx = np.mgrid[0:p, 0:p]
    board = np.where((yy + xx) % 2 == 0, a, b).astype(F)
    frame = np.zeros((p, p, 14), F)
    alb = F(1.0) - pm.EPS
    assert pm.EPS + alb == F(1.0)  # so that the pre-processed colour is the colour
    frame[..., 6:9] = alb
    for c in range(6):
        frame[..., c] = board
    res = pm.scores(frame, [(0, 0)], p)[0]
    bc = max(float(b), 0.0)
    assert res["var_normal"] == (float(a) - float(b)) ** 2 / 4 and res["var_colour"] == (float(a) - bc) ** 2 / 4
    assert res["score"] == res["var_colour"] + res["var_normal"]


def test_a_saturated_patch_scores_zero_and_its_sums_stay_inside_64_bits_at_the_largest_patch():
    """Bounds in Python integers, for P = 1024: every value at the clamp (the largest |q|), and the largest ah, al apart."""
    n = 3 * 1024 * 1024
    q = int(np.floor(float(pm.X_MAX) * pm.Q))
    assert q == 65504 << 20 and pm.population_sums(np.full(5, pm.X_MAX))[0] == 5 * q == -pm.population_sums(np.full(5, -pm.X_MAX))[0]
    ah, al = q >> 18, q & ((1 << 18) - 1)
    sums = (n * q, n * ah * ah, n * ah * al, n * al * al)
    assert sums[0] < 2 ** 63 and max(sums[1:]) < 2 ** 64
    res = pm.derive(sums + sums, n)
    assert res["score"] == 0.0 and res["var_colour"] == 0.0
    # the largest parts any value can have: ah of the clamp, al = 2^18 - 1
    ah_max, al_max = ah, (1 << 18) - 1
    assert n * max(ah_max * ah_max, ah_max * al_max, al_max * al_max) < 2 ** 64
    # the numerator N S2 - S1^2 and its two terms fit 128 bits
    assert n * ((sums[1] << 36) + (sums[2] << 19) + sums[3]) < 2 ** 128 and sums[0] ** 2 < 2 ** 127
    # a small patch of saturated values through the arrays: infinities and values above the clamp are the clamp
    frame = np.full((4, 4, 14), np.inf, F)
    frame[..., 6:9] = 0.0
    frame[..., 3:6] = -np.inf
    res = pm.scores(frame, [(0, 0)], 4)[0]
    assert res["score"] == 0.0 and res["colour_s1"] == 48 * q and res["normal_s1"] == -48 * q


# ---- the model against the reference's float64 measure ------------------------------------------------------------------

def bound(pre, corner, p):
    """|score - twin| <= sum over the two populations of [quantisation + NumPy's float64 rounding] + the model's own roundings.
    Quantisation: the floor moves a value by less than 2^-20, that is by at most 2^-21 around a common shift, so the standard
    deviation moves by at most 2^-21 and |var' - var| <= 2^-21 (2 sd + 2^-21).  NumPy: np.var forms a mean (n adds, each
    relative 2^-53 of a partial sum <= n M), n deviations |d| <= 2 M each off by at most (n + 2) 2^-53 M, their squares and the
    sum of those: at most (8 n + 16) 2^-53 M^2 in all, M the largest magnitude of the population.  The model: one conversion,
    two divisions and one addition in double, 4 x 2^-53 relative."""
    x, y = corner
    patch = pre[y:y + p, x:x + p].astype(np.float64)
    n = 3 * p * p
    total = 0.0
    for pop in (patch[..., 0:3], patch[..., 3:6]):
        sd, m = float(np.std(pop)), float(np.abs(pop).max())
        total += 2.0 ** -21 * (2.0 * sd + 2.0 ** -21) + (8 * n + 16) * 2.0 ** -53 * m * m + 4 * 2.0 ** -53 * sd * sd
    return total


def _worst_ratio(frames, sizes):
    worst = 0.0
    for frame in frames:
        pre = pm.preprocess(frame)
        assert np.isfinite(pre).all() and pre[..., 0:3].min() >= 0 and pre[..., 0:3].max() < 65504 and np.abs(pre[..., 3:6]).max() < 65504
        h, w = frame.shape[:2]
        for p in sizes:
            for corner in pm.corner_list(w, h, p):
                got = pm.score(pre, corner, p)
                tc, tn = pm.twin(pre, corner, p)
                err, lim = abs(got["score"] - (tc + tn)), bound(pre, corner, p)
                assert err <= lim, (w, h, p, corner, got["score"], tc + tn, err, lim)
                worst = max(worst, err / lim)
    return worst


def test_the_model_stays_within_the_bound_of_the_float64_measure_on_random_frames():
    """The generator's frames without the planted values: there sanitising changes nothing and the twin is the reference's
    measure itself."""
    frames = [pm.frame_pair(w, h, seed, specials=False)[0] for (w, h) in ((37, 29), (64, 48)) for seed in range(4)]
    worst = _worst_ratio(frames, (1, 5, 8, 16, 29))
    print(f"random: largest |score - twin| / bound = {worst:.3g}")
    assert 0.0 < worst <= 1.0


def test_the_model_stays_within_the_bound_of_the_float64_measure_on_the_oracle_frames():
    names = ("oracle_64_spp1_xorwow.npz", "oracle_64_spp4_xorwow.npz", "oracle_64_spp4_philox.npz", "oracle_64_spp16_xorwow_glm_b8.npz")
    frames = [np.load(os.path.join(GOLDEN, n))["image"] for n in names]
    worst = _worst_ratio(frames, (8, 16, 64))
    print(f"oracle: largest |score - twin| / bound = {worst:.3g}")
    assert 0.0 < worst <= 1.0


# ---- pick_patches ---------------------------------------------------------------------------------------------------

def test_pick_patches_returns_distinct_indices_and_repeats_with_the_seed(pt):
    scores = [float(v) for v in np.random.default_rng(4).uniform(0.0, 3.0, 64)]
    a = pt.pick_patches(scores, 16, random.Random(7))
    assert len(a) == 16 == len(set(a)) and all(0 <= k < 64 for k in a)
    assert pt.pick_patches(scores, 16, random.Random(7)) == a
    assert pt.pick_patches(scores, 16, random.Random(8)) != a
    assert sorted(pt.pick_patches(scores, 64, random.Random(1))) == list(range(64))  # (all of them, in some order)


def test_pick_patches_with_all_zero_scores_takes_where_the_scan_stands(pt):
    """No candidate is ever taken by chance, so the first take is the unconditional one: after 10 n + 1 candidates have been
    passed over, at position (10 n + 1) mod candidates of the scan; every scan after it starts at the front.  With 10 n + 1
    candidates (or a divisor of it) that is [0, 1, ..., n - 1]; with the 4 n of training_patches it is 2 n + 1 first."""
    for n in (1, 2, 4):
        assert pt.pick_patches([0.0] * (10 * n + 1), n, random.Random(3)) == list(range(n))
    assert pt.pick_patches([0.0] * 3, 2, random.Random(3)) == [0, 1]
    assert pt.pick_patches([0.0] * 16, 4, random.Random(3)) == [9, 0, 1, 2]


def test_pick_patches_takes_the_candidate_that_holds_all_of_the_total_first(pt):
    for seed in range(5):
        picks = pt.pick_patches([0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 0.0], 2, random.Random(seed))
        assert picks[0] == 2 and picks[1] != 2


def test_pick_patches_refuses_more_than_there_are(pt):
    with pytest.raises(ValueError):
        pt.pick_patches([1.0, 2.0], 3, random.Random(0))
    assert pt.pick_patches([], 0, random.Random(0)) == []


# ---- the C++ wrapper ------------------------------------------------------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include "PatchSampler.h"
int main() {
  PatchSampler ok_to_name(0, 64, 16, 4);  // width 0: the create fails, GPUassert prints and exits
  std::printf("not reached\n");
  return 0;
}
"""


def test_patch_sampler_compiles_alone_and_fails_with_the_message(pt, tmp_path):
    src, exe = tmp_path / "sampler.cpp", str(tmp_path / "sampler")
    src.write_text(PROGRAM)
    libdir = os.path.dirname(pt.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "cuda-pathtrace_amd", "host"), "-o", exe,
                           str(src), "-L", libdir, "-lptcore", f"-Wl,-rpath,{libdir}"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode != 0 and "not reached" not in run.stdout
    assert "GPUassert" in run.stderr and "pt_patches_create" in run.stderr and "width 0" in run.stderr
