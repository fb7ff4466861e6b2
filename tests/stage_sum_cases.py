"""Cases that take the second-level reductions of the three post-process stages past their first stride: tone mapping's
adapt_kernel (csrc/pt_tonemap.hip), frame comparison's sum_kernel (csrc/pt_compare.hip) and the training patches' max_kernel,
gather fold and sum_kernel (csrc/pt_patches.hip).  Each of them folds its partials with a loop of stride BLOCK = 256; the stages'
own test files stop at sizes where that loop makes one trip.  Two kinds of case: random frames held to the NumPy models
(tonemap_model, compare_model, patches_model), and PLACED frames whose answer follows from how they were built -- Python
integers and single float32 operations -- so that a partial lost in a later trip changes a number known beforehand.
tests/test_stage_sums_host.py holds the models to the placed answers and the sizes to the trips they claim;
tests/test_stage_sums_gpu.py holds the kernels to both.  Every builder is computed once (lru_cache) and hands out read-only
arrays."""
import functools
import os
import re

import numpy as np

import compare_model as cm
import patches_model as pm
import tonemap_model as tm

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-pathtrace_amd", "csrc")

# What the cases were made for; tests/test_stage_sums_host.py reads the same names out of the three sources.
BLOCK, TILE, SCORE_PIXELS, MAX_PARTS = 256, 16, 1024, 256
FIRST_TRIP = BLOCK * BLOCK  # pixels that the first trip of a 256-workgroup, 256-lane loop reaches


def hip_constant(source, name):
    """`constexpr int NAME = <number or another constant>;` of csrc/<source> as an int."""
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(r"^constexpr int %s = (\w+);" % re.escape(name), text, re.M)
    assert m, f"{source}: no constexpr int {name}"
    return int(m.group(1)) if m.group(1).isdigit() else hip_constant(source, m.group(1))


def ceil_div(a, b):
    return -(-a // b)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def picks(n):
    """The partials a one-per-frame case lights: both ends of the first trip, the start of the second, both ends of the second
    lane-for-lane, the start of the third, the last."""
    return [0, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, n - 1]


# The class a size claims for its number of partials n: "over": n > BLOCK (a second trip for some lanes); "double": n == 2 BLOCK
# (exactly two trips for every lane); "triple": n > 2 BLOCK (a third trip).
CLASSES = {"over": lambda n, block: n > block, "double": lambda n, block: n == 2 * block, "triple": lambda n, block: n > 2 * block}

# ---- tone mapping ------------------------------------------------------------------------------------------------------------

TONEMAP_SIZES = [((257, 256), "over"), ((512, 256), "double"), ((513, 256), "triple"), ((1031, 67), "over")]  # (w, h): 257, 512, 513, 270 blocks
TONEMAP_BATCH_SIZE = (513, 256)
TONEMAP_LIT_SIZE = (527, 263)  # 542 blocks, the last one of 105 pixels


def tonemap_blocks(w, h, block=BLOCK):
    return ceil_div(w * h, block)


@functools.lru_cache(maxsize=None)
def tonemap_random(w, h, stride):
    """-> (frame, the model's bytes, the model's exposure) with the defaults: ACES, sRGB, metered."""
    frame = tm.random_frame(w, h, stride, seed=w * 131 + h + stride)
    want, exps = tm.tonemap_sequence([frame])
    return frozen(frame, want[0]) + (exps[0],)


def grey_exposure(g, key=0.18):
    """The exposure of a frame whose metered pixels are all the grey g: key / lum(g, g, g), one float32 division."""
    return F(key) / tm.lum(np.full(3, g, F))


@functools.lru_cache(maxsize=None)
def tonemap_two_populations():
    """513 x 256: the pixels the first trip reaches are grey 2^-4, the rest grey 2^4.  -> (frame [H][W][3], exposure): the
    exposure from Python integers over the two luminances' bits; it is neither population's own."""
    w, h = TONEMAP_BATCH_SIZE
    n = w * h
    lo, hi = F(2.0 ** -4), F(2.0 ** 4)
    frame = np.empty((n, 3), F)
    frame[:FIRST_TRIP], frame[FIRST_TRIP:] = lo, hi
    b_lo, b_hi = (tm.scalar_bits(tm.lum(np.full(3, g, F))) for g in (lo, hi))
    assert tm.METER_MIN <= b_lo <= tm.METER_MAX and tm.METER_MIN <= b_hi <= tm.METER_MAX
    S, K = FIRST_TRIP * b_lo + (n - FIRST_TRIP) * b_hi, n
    e = F(0.18) / tm.from_bits(np.uint32(S // K))
    assert len({tm.scalar_bits(x) for x in (e, grey_exposure(lo), grey_exposure(hi))}) == 3, "a dropped trip would not show"
    return frozen(frame.reshape(h, w, 3)), F(e)


@functools.lru_cache(maxsize=None)
def tonemap_lit_blocks():
    """527 x 263, seven frames: frame k is zero (nothing to meter) but for the pixels of block picks(blocks)[k], which hold grey
    2^-k.  -> (frames [7][H][W][3], blocks lit, exposures): exposure k = key / lum(2^-k), whatever came before (adapt 1)."""
    w, h = TONEMAP_LIT_SIZE
    n = w * h
    lit = picks(tonemap_blocks(w, h))
    frames = np.zeros((len(lit), n, 3), F)
    for k, t in enumerate(lit):
        frames[k, t * BLOCK:min((t + 1) * BLOCK, n)] = F(2.0 ** -k)
    exps = [grey_exposure(F(2.0 ** -k)) for k in range(len(lit))]
    assert len({tm.scalar_bits(e) for e in exps} | {tm.scalar_bits(F(1.0))}) == len(lit) + 1  # a lost block keeps the exposure before
    return frozen(frames.reshape(len(lit), h, w, 3)), lit, exps


@functools.lru_cache(maxsize=None)
def tonemap_batch():
    """Three 513 x 256 frames (stride 14) whose brightness steps by x 8, through one session at adapt 0.5.  -> (frames, the
    model's bytes, the model's exposures)."""
    w, h = TONEMAP_BATCH_SIZE
    frames = tm.stepped_frames(w, h, 14, 3, seed=13)
    want, exps = tm.tonemap_sequence(frames, rate=0.5)
    assert len({tm.scalar_bits(e) for e in exps}) == 3
    return frozen(frames), want, exps


# ---- frame comparison --------------------------------------------------------------------------------------------------------

COMPARE_SIZES = [((4112, 1), "over"), ((16, 4097), "over"), ((272, 272), "over"), ((527, 263), "triple")]  # 257, 257, 289, 561 tiles
COMPARE_PLACED_SIZES = [(272, 272), (527, 263)]
COMPARE_BATCH_SIZE = (272, 272)
COMPARE_PICK_SIZE = (527, 263)
CHECKER_SIZES = [(37, 29), (272, 272)]
COMPARE_STRIDES = (14, 3)
QUARTER = 1 << 32  # floor(0.25 x 2^34): the quantised m of one channel that differs by 0.5


def compare_tiles(w, h, tile=TILE):
    return ceil_div(w, tile), ceil_div(w, tile) * ceil_div(h, tile)


def tile_origin(t, w):
    """(x, y) of the first pixel of tile t."""
    tx = ceil_div(w, TILE)
    return (t % tx) * TILE, (t // tx) * TILE


@functools.lru_cache(maxsize=None)
def compare_random(w, h):
    """-> (img stride 14, ref stride 3, the model's result) of the stages' own random pair at this size."""
    img, ref = cm.hdr_pair(w, h, seed=w * 7 + h, img_stride=COMPARE_STRIDES[0], ref_stride=COMPARE_STRIDES[1])
    return frozen(img, ref) + (model_compare(img, ref),)


def model_compare(img, ref):
    want = cm.compare(img, ref)
    frozen(want["m"], want["r"], want["s"])
    return want


@functools.lru_cache(maxsize=None)
def compare_one_pixel_per_tile(w, h):
    """ref 0.25 everywhere; img = ref but for channel 0 = 0.75 in the first pixel of every tile: m = 0.25 there and 0 elsewhere.
    -> (img, ref, {"sum_mse": tiles << 32})."""
    ref = np.full((h, w, 3), 0.25, F)
    img = ref.copy()
    img[::TILE, ::TILE, 0] = 0.75
    return frozen(img, ref) + ({"sum_mse": compare_tiles(w, h)[1] * QUARTER},)


@functools.lru_cache(maxsize=None)
def compare_counts_per_tile(w, h):
    """The first pixel of every tile: a NaN in img channel 1 (one non-finite pixel), and img channel 2 = 4.0 against ref channel
    2 = 0.0 (16 / 0.01 reaches the cap: one saturated channel).  -> (img, ref, {"nonfinite": tiles, "saturated": tiles})."""
    ref = np.full((h, w, 3), 0.25, F)
    img = ref.copy()
    img[::TILE, ::TILE, 1] = np.nan
    img[::TILE, ::TILE, 2] = 4.0
    ref[::TILE, ::TILE, 2] = 0.0
    tiles = compare_tiles(w, h)[1]
    return frozen(img, ref) + ({"nonfinite": tiles, "saturated": tiles},)


@functools.lru_cache(maxsize=None)
def compare_one_tile_per_frame():
    """527 x 263, seven images against ONE reference (0.25 everywhere): image k differs in one pixel, the first of tile
    picks(tiles)[k], by 0.5 in channel 0.  -> (imgs [7][H][W][3], ref, tiles lit): every sum_mse is 1 << 32 and every m is 0 but
    for the 0.25 of that pixel."""
    w, h = COMPARE_PICK_SIZE
    lit = picks(compare_tiles(w, h)[1])
    ref = np.full((h, w, 3), 0.25, F)
    imgs = np.repeat(ref[None], len(lit), axis=0)
    for k, t in enumerate(lit):
        x, y = tile_origin(t, w)
        imgs[k, y, x, 0] = 0.75
    return frozen(imgs, ref) + (lit,)


@functools.lru_cache(maxsize=None)
def compare_checkerboard(w, h):
    """The checkerboard (x + y) & 1 in all three channels against its inverse: anticorrelated everywhere, so the model's s is
    negative in every pixel and the signed sum is negative.  -> (img, ref, the model's result)."""
    yy, xx = np.mgrid[0:h, 0:w]
    c = ((xx + yy) & 1).astype(F)
    img = np.repeat(c[..., None], 3, axis=2)
    ref = F(1.0) - img
    want = model_compare(img, ref)
    assert want["s"].max() < 0 and want["sum_ssim"] < 0 and want["ssim"] < 0
    return frozen(img, ref) + (want,)


@functools.lru_cache(maxsize=None)
def compare_batch():
    """Three random 272 x 272 pairs (strides 14 and 3).  -> (imgs [3][H][W][14], refs [3][H][W][3], the model's results)."""
    w, h = COMPARE_BATCH_SIZE
    pairs = [cm.hdr_pair(w, h, seed=60 + k, img_stride=COMPARE_STRIDES[0], ref_stride=COMPARE_STRIDES[1]) for k in range(3)]
    imgs, refs = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    return frozen(imgs, refs) + ([model_compare(a, b) for a, b in pairs],)


# ---- training patches --------------------------------------------------------------------------------------------------------

PATCH_FRAME = (520, 516)  # 268 320 pixels: 1049 blocks -> MAX_PARTS workgroups, five trips each
BIG_PATCH = 513           # 258 score workgroups per patch; 5 staging runs per row, 2565 units over 256 workgroups of the gather
BIG_CORNERS = ((0, 0), (7, 3))
SMALL_PATCH = 8
# channel -> the pixel index of its strict maximum: the start of the second trip, the last pixel, the end of the first trip
# (workgroup 255: wave 3 of the gather's fold), pixel 0, and lane 5 of the third trip
PLANTED = {9: FIRST_TRIP, 10: PATCH_FRAME[0] * PATCH_FRAME[1] - 1, 11: FIRST_TRIP - 1, 12: 0, 13: 2 * FIRST_TRIP + 5}
PLANTED_VALUES = {9: 900.0, 10: 70.0, 11: 50.0, 12: 30.0, 13: 10.0}
# P = 8 corners around and between the planted pixels (0, 0), (15, 126), (16, 126), (37, 252) and (519, 515), none holding one
PLANTED_CORNERS = ((1, 0), (511, 508), (512, 0), (0, 508), (1, 1), (3, 2), (1, 1), (2, 1), (511, 505), (257, 254), (17, 120), (7, 119),
                   (38, 252))


def patch_parts(w, h, block=BLOCK, max_parts=MAX_PARTS):
    """(workgroups of max_kernel, trips of its grid-stride loop)."""
    parts = min(ceil_div(w * h, block), max_parts)
    return parts, ceil_div(w * h, parts * block)


def patch_chunks(p, score_pixels=SCORE_PIXELS):
    return ceil_div(p * p, score_pixels)


def small_corners():
    return pm.corner_list(*PATCH_FRAME, SMALL_PATCH)


@functools.lru_cache(maxsize=None)
def patches_random():
    """The stages' own random pair at 520 x 516 (a NaN in each of channels 9-13 too).  -> (frame, gt stride 3)."""
    w, h = PATCH_FRAME
    return frozen(*pm.frame_pair(w, h, seed=w * 7 + h, gt_stride=3, nan_features=True))


@functools.lru_cache(maxsize=None)
def patches_model(case, p, corners):
    """case: "random" | "planted" | "normal".  -> (the model's results, inputs, targets) for the corners at patch size p."""
    frame, gt = {"random": patches_random, "planted": patches_planted, "normal": patches_constant_normal}[case]()[:2]
    return (pm.scores(frame, corners, p),) + frozen(*pm.gather(frame, gt, corners, p))


@functools.lru_cache(maxsize=None)
def patches_planted():
    """A random pair whose channels 9-13 take their strict maxima at PLANTED, every other value of a channel at most half its
    maximum.  -> (frame, gt, divisors [5]): divisor k = (float)(0.00316 + (double)PLANTED_VALUES[9 + k])."""
    w, h = PATCH_FRAME
    frame, gt = pm.frame_pair(w, h, seed=77, gt_stride=3)
    flat = frame.reshape(w * h, 14)
    flat[:, 10:14] = np.minimum(flat[:, 10:14], F(4.0))
    for c, i in PLANTED.items():
        flat[i, c] = PLANTED_VALUES[c]
    for c, i in PLANTED.items():
        others = np.delete(flat[:, c], i)
        assert 0 <= i < w * h and flat[i, c] == F(PLANTED_VALUES[c]) and others.max() <= flat[i, c] / 2 and np.isfinite(others).all()
    held = {(i % w, i // w) for i in PLANTED.values()}
    for x, y in PLANTED_CORNERS:
        assert 0 <= x <= w - SMALL_PATCH and 0 <= y <= h - SMALL_PATCH
        assert not any(x <= px < x + SMALL_PATCH and y <= py < y + SMALL_PATCH for px, py in held), (x, y)
    div = np.array([F(0.00316 + PLANTED_VALUES[c]) for c in range(9, 14)], F)
    return frozen(frame, gt, div)


@functools.lru_cache(maxsize=None)
def patches_constant_normal():
    """Normal (1, 0, 0) everywhere, colour 0, albedo 0.5, noise in channels 9-13.  -> (frame, gt, the eight sums of any P = 513
    patch): the normal's population is P^2 values of 1.0 (q = 2^20: high part 4, low part 0) and 2 P^2 zeros."""
    w, h = PATCH_FRAME
    rng = np.random.default_rng(3)
    frame = np.zeros((h, w, 14), F)
    frame[..., 3] = 1.0
    frame[..., 6:9] = 0.5
    frame[..., 9:14] = rng.uniform(0.0, 2.0, (h, w, 5))
    gt = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    pp = BIG_PATCH * BIG_PATCH
    sums = dict(zip(pm.SUMS, (0, 0, 0, 0, pp << 20, 16 * pp, 0, 0)))
    return frozen(frame, gt) + (sums,)
