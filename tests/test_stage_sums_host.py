"""CPU side of tests/stage_sum_cases.py: every size takes the trips it claims by the constants read out of the three sources (a
changed BLOCK, TILE, SCORE_PIXELS or MAX_PARTS fails here instead of silently moving the cases back under one trip), the builders'
own conditions hold, and every PLACED answer is the answer the NumPy models give -- so that tests/test_stage_sums_gpu.py holds
the kernels to a construction and to a model that agree."""
import numpy as np
import pytest

import compare_model as cm
import patches_model as pm
import stage_sum_cases as sc
import tonemap_model as tm

F = np.float32
TM_BLOCK = sc.hip_constant("pt_tonemap.hip", "BLOCK")
CMP_BLOCK, CMP_TILE = sc.hip_constant("pt_compare.hip", "BLOCK"), sc.hip_constant("pt_compare.hip", "TILE")
PAT_BLOCK, PAT_PARTS = sc.hip_constant("pt_patches.hip", "BLOCK"), sc.hip_constant("pt_patches.hip", "MAX_PARTS")
PAT_SCORE = sc.hip_constant("pt_patches.hip", "SCORE_PIXELS")


def _picks_cover(lit, n, block):
    assert len(set(lit)) == len(lit) and all(0 <= t < n for t in lit), (lit, n)
    assert {0, block - 1, block, block + 1, 2 * block - 1, 2 * block, n - 1} == set(lit) and n - 1 > 2 * block


# ---- the sizes ---------------------------------------------------------------------------------------------------------------

def test_the_cases_were_made_for_the_sources_constants():
    assert (TM_BLOCK, CMP_BLOCK, PAT_BLOCK) == (sc.BLOCK,) * 3 and CMP_TILE == sc.TILE
    assert PAT_PARTS == sc.MAX_PARTS == PAT_BLOCK and PAT_SCORE == sc.SCORE_PIXELS and sc.FIRST_TRIP == PAT_PARTS * PAT_BLOCK


@pytest.mark.parametrize("size, cls", sc.TONEMAP_SIZES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_tonemap_sizes_take_the_trips_they_claim(size, cls):
    assert sc.CLASSES[cls](sc.tonemap_blocks(*size, TM_BLOCK), TM_BLOCK)


def test_tonemap_sizes_cover_every_class_and_a_ragged_block():
    assert {c for _, c in sc.TONEMAP_SIZES} == set(sc.CLASSES)
    assert sc.tonemap_blocks(257, 256, TM_BLOCK) == TM_BLOCK + 1 and sc.tonemap_blocks(513, 256, TM_BLOCK) == 2 * TM_BLOCK + 1
    assert (1031 * 67) % TM_BLOCK != 0
    assert sc.CLASSES["triple"](sc.tonemap_blocks(*sc.TONEMAP_BATCH_SIZE, TM_BLOCK), TM_BLOCK)
    w, h = sc.TONEMAP_LIT_SIZE
    _picks_cover(sc.tonemap_lit_blocks()[1], sc.tonemap_blocks(w, h, TM_BLOCK), TM_BLOCK)
    assert (w * h) % TM_BLOCK != 0  # the last lit block is ragged


@pytest.mark.parametrize("size, cls", sc.COMPARE_SIZES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_compare_sizes_take_the_trips_they_claim(size, cls):
    assert sc.CLASSES[cls](sc.compare_tiles(*size, CMP_TILE)[1], CMP_BLOCK)


def test_compare_sizes_cover_one_row_one_column_and_ragged_tiles():
    assert sc.compare_tiles(4112, 1, CMP_TILE) == (CMP_BLOCK + 1, CMP_BLOCK + 1)
    assert sc.compare_tiles(16, 4097, CMP_TILE) == (1, CMP_BLOCK + 1)
    assert sc.compare_tiles(527, 263, CMP_TILE) == (33, 561) and 527 % CMP_TILE and 263 % CMP_TILE
    for size in sc.COMPARE_PLACED_SIZES + [sc.COMPARE_BATCH_SIZE, sc.CHECKER_SIZES[1]]:
        assert sc.compare_tiles(*size, CMP_TILE)[1] > CMP_BLOCK
    assert sc.CLASSES["triple"](sc.compare_tiles(*sc.COMPARE_PLACED_SIZES[1], CMP_TILE)[1], CMP_BLOCK)
    _picks_cover(sc.compare_one_tile_per_frame()[2], sc.compare_tiles(*sc.COMPARE_PICK_SIZE, CMP_TILE)[1], CMP_BLOCK)


def test_patch_sizes_take_the_trips_they_claim():
    w, h = sc.PATCH_FRAME
    assert sc.patch_parts(w, h, PAT_BLOCK, PAT_PARTS) == (PAT_PARTS, 5)
    assert sc.patch_chunks(sc.BIG_PATCH, PAT_SCORE) == 258 > PAT_BLOCK and sc.patch_chunks(256, PAT_SCORE) <= PAT_BLOCK
    run = sc.hip_constant("pt_patches.hip", "RUN")
    assert sc.ceil_div(sc.BIG_PATCH, run) * sc.BIG_PATCH == 2565  # units of the gather over at most 256 workgroups: 10 full trips and more
    for x, y in sc.BIG_CORNERS + tuple(sc.small_corners()):
        assert 0 <= x and 0 <= y
    assert sc.BIG_CORNERS[1] == (w - sc.BIG_PATCH, h - sc.BIG_PATCH)
    # where max_kernel meets each planted pixel: (trip, workgroup); the gather folds workgroup 64 w + l in wave w
    where = {c: (i // sc.FIRST_TRIP, (i // PAT_BLOCK) % PAT_PARTS) for c, i in sc.PLANTED.items()}
    assert where == {9: (1, 0), 10: (4, 24), 11: (0, 255), 12: (0, 0), 13: (2, 0)}
    assert where[11][1] >= 192  # wave 3 of the gather's fold


# ---- random pairs: what the parity cases must contain ------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [s for s, _ in sc.COMPARE_SIZES], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_compare_pairs_have_both_counts(size):
    want = sc.compare_random(*size)[2]
    assert want["saturated"] > 0 and want["nonfinite"] > 0 and want["sum_mse"] > 0 and want["pixels"] == size[0] * size[1]


# ---- placed answers against the models ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", sc.COMPARE_PLACED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_pixel_per_tile_sums_to_the_tile_count(size):
    img, ref, expect = sc.compare_one_pixel_per_tile(*size)
    want = cm.compare(img, ref)
    tiles = sc.compare_tiles(*size)[1]
    assert expect["sum_mse"] == tiles << 32 == want["sum_mse"] and want["saturated"] == want["nonfinite"] == 0
    assert np.count_nonzero(want["m"]) == tiles and (want["m"][::sc.TILE, ::sc.TILE] == F(0.25)).all()
    img, ref, expect = sc.compare_counts_per_tile(*size)
    want = cm.compare(img, ref)
    assert (want["nonfinite"], want["saturated"]) == (tiles, tiles) == (expect["nonfinite"], expect["saturated"])


def test_one_tile_per_frame_sums_to_one_quarter():
    imgs, ref, lit = sc.compare_one_tile_per_frame()
    w, h = sc.COMPARE_PICK_SIZE
    for k, t in enumerate(lit):
        want = cm.compare(imgs[k], ref)
        x, y = sc.tile_origin(t, w)
        assert want["sum_mse"] == sc.QUARTER and np.flatnonzero(want["m"]).tolist() == [y * w + x] and want["m"][y, x] == F(0.25)
        assert np.flatnonzero(want["r"]).tolist() == [y * w + x]
    assert len({sc.tile_origin(t, w) for t in lit}) == len(lit)


@pytest.mark.parametrize("size", sc.CHECKER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_checkerboard_against_its_inverse_has_a_negative_sum(size):
    _, _, want = sc.compare_checkerboard(*size)
    assert want["s"].max() < 0 and want["sum_ssim"] < 0 and want["sum_ssim"] == int(np.floor(want["s"].astype(np.float64) * cm.QS).sum())
    assert want["ssim"] == want["sum_ssim"] / cm.QS / (size[0] * size[1]) < -0.99  # (-0.99572 at 37 x 29, -0.99640 at 272 x 272)


def test_two_populations_meter_to_the_constructed_exposure():
    frame, e = sc.tonemap_two_populations()
    _, exps = tm.tonemap_sequence([frame])
    assert tm.scalar_bits(exps[0]) == tm.scalar_bits(e)
    first = frame.reshape(-1, 3)[:sc.FIRST_TRIP]
    assert tm.scalar_bits(tm.tonemap_sequence([first[None]])[1][0]) == tm.scalar_bits(sc.grey_exposure(F(2.0 ** -4))) != tm.scalar_bits(e)


def test_lit_blocks_meter_to_their_own_grey():
    frames, lit, exps = sc.tonemap_lit_blocks()
    _, got = tm.tonemap_sequence(frames, rate=1.0)
    assert [tm.scalar_bits(e) for e in got] == [tm.scalar_bits(e) for e in exps]
    n = frames[0].size // 3
    for k, t in enumerate(lit):
        S, K = tm.meter(frames[k])
        assert K == min(sc.BLOCK, n - t * sc.BLOCK) and S == K * tm.scalar_bits(tm.lum(np.full(3, 2.0 ** -k, F)))
        assert tm.meter(np.delete(frames[k].reshape(-1, 3), np.s_[t * sc.BLOCK:(t + 1) * sc.BLOCK], axis=0)) == (0, 0)


def test_planted_maxima_give_the_constructed_divisors():
    frame, gt, div = sc.patches_planted()
    assert np.array_equal(pm.bits(pm.divisors(frame)), pm.bits(div))
    flat = frame.reshape(-1, 14)
    for c, i in sc.PLANTED.items():
        assert int(np.argmax(flat[:, c])) == i and np.count_nonzero(flat[:, c] == flat[i, c]) == 1
    # without any one of the planted pixels the divisor is another float: a lost trip or wave shows in every gathered value
    for c, i in sc.PLANTED.items():
        assert pm.divisors(np.delete(flat, i, axis=0)[None])[c - 9] != div[c - 9]
    _, inputs, _ = sc.patches_model("planted", sc.SMALL_PATCH, sc.PLANTED_CORNERS)
    with np.errstate(all="ignore"):
        for k, (x, y) in enumerate(sc.PLANTED_CORNERS):
            crop = frame[y:y + sc.SMALL_PATCH, x:x + sc.SMALL_PATCH, 9:14] / div
            assert np.array_equal(pm.bits(inputs[k, 9:14]), pm.bits(crop.transpose(2, 0, 1)))


def test_constant_normal_has_the_constructed_sums():
    _, _, sums = sc.patches_constant_normal()
    pp = sc.BIG_PATCH ** 2
    assert (sums["normal_s1"], sums["normal_a"], sums["normal_b"], sums["normal_c"]) == (pp * 2 ** 20, 16 * pp, 0, 0)
    for want in sc.patches_model("normal", sc.BIG_PATCH, sc.BIG_CORNERS)[0]:
        assert {k: want[k] for k in pm.SUMS} == sums and want["values"] == 3 * pp and want["var_colour"] == 0.0
        assert want["var_normal"] == 2.0 / 9.0  # the variance of (1, 0, 0): exact integers up to the one conversion
