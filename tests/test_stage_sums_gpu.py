"""The second-level reductions of tone mapping, frame comparison and training patches past their first stride, on the product
library (tests/stage_sum_cases.py): adapt_kernel above 256, 512 and 513 blocks, the comparison's sum_kernel above 256 and 512
tiles, the patches' max_kernel over five trips, the gather's fold of all 256 partial maxima and the patches' sum_kernel above 256
chunks.  Random frames are held bit for bit to the NumPy models; placed frames first to the answer their construction gives
(tests/test_stage_sums_host.py holds the models to the same answers), then to the models; batches to their singles at sizes where
the per-frame offsets f * blocks, f * tiles and patch * chunks exceed a stride; guard bands and inputs keep their bytes.  Every
comparison is of bits or of integers: there is no tolerance in this file.  A failure names the stage, the size and the first
field that is wrong."""
import numpy as np
import pytest

import compare_model as cm
import patches_model as pm
import stage_sum_cases as sc
import tonemap_model as tm
from test_patches_gpu import Rig  # a session with its pair on the device and two outputs between guard bands

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64  # words on either side of an output
CMP_INTS = ("sum_mse", "sum_relmse", "sum_ssim", "pixels", "saturated", "nonfinite")
CMP_DOUBLES = ("mse", "rms", "psnr", "relmse", "ssim")
COMPARED = [0]


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    print(f"\ntest_stage_sums_gpu: {COMPARED[0]} values compared with their expectation")


def _ids(s):
    return f"{s[0]}x{s[1]}"


# ---- tone mapping ------------------------------------------------------------------------------------------------------------

def _tm_exposure(got, want, what):
    COMPARED[0] += 1
    assert tm.scalar_bits(got) == tm.scalar_bits(want), (f"tonemap {what}: exposure {float(got)!r} (bits {tm.scalar_bits(got):#x}) on the "
                                                         f"device, {float(want)!r} (bits {tm.scalar_bits(want):#x}) expected")


def _tm_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, f"tonemap {what}: shape"
    COMPARED[0] += got.size
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (f"tonemap {what}: bytes: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])].tolist()} on the device, {want[tuple(bad[0])].tolist()} expected")


def _tonemap_once(pt, frame, **opts):
    """One frame through a fresh session -> (bytes [H][W][4], exposure)."""
    h, w = frame.shape[:2]
    t = pt.Tonemap(w, h, **opts)
    try:
        return pt.tonemap_frame(frame, tonemap=t), t.exposure()
    finally:
        t.destroy()


@pytest.mark.parametrize("stride", [14, 3])
@pytest.mark.parametrize("size", [s for s, _ in sc.TONEMAP_SIZES], ids=_ids)
def test_tonemap_random_frames_equal_the_model(pt, gpu, size, stride):
    """257, 512, 513 and 270 blocks: the metered exposure and the bytes of the default curve and encode."""
    w, h = size
    frame, want, e = sc.tonemap_random(w, h, stride)
    got, ge = _tonemap_once(pt, frame)
    what = f"{w}x{h} ({sc.tonemap_blocks(w, h)} blocks) random, stride {stride}"
    _tm_exposure(ge, e, what)
    _tm_bytes(got, want, what)


def test_tonemap_two_populations_meter_across_the_trips(pt, gpu):
    """The first trip's pixels are grey 2^-4, the later trips' grey 2^4: the exposure is the integer mean over both."""
    frame, e = sc.tonemap_two_populations()
    got, ge = _tonemap_once(pt, frame)
    what = f"{_ids(sc.TONEMAP_BATCH_SIZE)} two populations"
    _tm_exposure(ge, e, what + ", constructed")
    _tm_bytes(got, tm.map_encode(frame, e), what + ", constructed exposure")
    want, exps = tm.tonemap_sequence([frame])
    _tm_exposure(ge, exps[0], what + ", model")
    _tm_bytes(got, want[0], what + ", model")


def test_tonemap_one_lit_block_per_frame(pt, gpu):
    """Seven frames in groups of two: the only metered pixels of frame k lie in one block (0, 255, 256, 257, 511, 512, the last),
    so exposure k is that block's grey's -- a lost block leaves the exposure of the frame before."""
    frames, lit, exps = sc.tonemap_lit_blocks()
    n, h, w = frames.shape[:3]
    want, mexps = tm.tonemap_sequence(frames, rate=1.0)
    t = pt.Tonemap(w, h, adapt=1.0, max_frames=2)
    d_src, d_out = pt.DeviceBuffer(frames.nbytes).upload(frames), pt.DeviceBuffer(n * w * h * 4)
    try:
        for k in range(n):  # frame by frame, where every exposure can be read
            t.run(d_src.ptr + k * frames[k].nbytes, d_out.ptr, pixel_stride=3)
            _tm_exposure(t.exposure(), exps[k], f"{w}x{h} lit block {lit[k]}, single {k}, constructed")
            assert tm.scalar_bits(mexps[k]) == tm.scalar_bits(exps[k])
        t.reset()
        t.run_frames(d_src.ptr, n, d_out.ptr, pixel_stride=3)
        out = d_out.download(np.uint8, (n, h, w, 4))
        for k in range(n):
            what = f"{w}x{h} lit block {lit[k]}, frame {k} of the batch"
            # the bytes carry the exposure: the lit grey maps to one code, the model's for the constructed exposure
            _tm_bytes(out[k], tm.map_encode(frames[k], exps[k]), what + ", constructed exposure")
            _tm_bytes(out[k], want[k], what + ", model")
        _tm_exposure(t.exposure(), exps[-1], f"{w}x{h} lit block {lit[-1]}, after the batch, constructed")
    finally:
        t.destroy()
        d_src.free()
        d_out.free()


def test_tonemap_batch_above_512_blocks_equals_its_singles(pt, gpu):
    """Three 513 x 256 frames at adapt 0.5 through max_frames 2 (groups of 2 and 1: partials at f * 513) against three single
    calls and the model; guard bands around the batch's output and the input keep their bytes."""
    frames, want, exps = sc.tonemap_batch()
    n, h, w = frames.shape[:3]
    px = w * h
    d_src, d_out = pt.DeviceBuffer(frames.nbytes).upload(frames), pt.DeviceBuffer((n * px + 2 * GUARD) * 4)
    try:
        singles = []
        t = pt.Tonemap(w, h, adapt=0.5)
        try:
            for k in range(n):
                t.run(d_src.ptr + k * frames[k].nbytes, d_out.ptr + (GUARD + k * px) * 4)
                _tm_exposure(t.exposure(), exps[k], f"{w}x{h} single {k}")
            singles = d_out.download(np.uint8, (n * px + 2 * GUARD, 4))[GUARD:-GUARD].reshape(n, h, w, 4)
        finally:
            t.destroy()
        for k in range(n):
            _tm_bytes(singles[k], want[k], f"{w}x{h} single {k}")
        t = pt.Tonemap(w, h, adapt=0.5, max_frames=2)
        try:
            pt.check(pt.lib.pt_memset(d_out.ptr, 0x5C, (n * px + 2 * GUARD) * 4))
            t.run_frames(d_src.ptr, n, d_out.ptr + GUARD * 4)
            raw = d_out.download(np.uint32, (n * px + 2 * GUARD,))
            _tm_exposure(t.exposure(), exps[-1], f"{w}x{h} batch of {n}, max_frames 2")
        finally:
            t.destroy()
        assert (raw[:GUARD] == 0x5C5C5C5C).all() and (raw[-GUARD:] == 0x5C5C5C5C).all(), f"tonemap {w}x{h} batch: guard band written"
        batch = raw[GUARD:-GUARD].view(np.uint8).reshape(n, h, w, 4)
        for k in range(n):
            _tm_bytes(batch[k], singles[k], f"{w}x{h} batch frame {k} against its single")
        assert d_src.download(F, frames.shape).tobytes() == frames.tobytes(), f"tonemap {w}x{h} batch: the input was written"
    finally:
        d_src.free()
        d_out.free()


# ---- frame comparison --------------------------------------------------------------------------------------------------------

def _cmp_result(got, want, what, fields=CMP_INTS + CMP_DOUBLES):
    for k in fields:
        COMPARED[0] += 1
        if k in CMP_INTS:
            assert got[k] == want[k], f"compare {what}: {k} {got[k]} on the device, {want[k]} expected"
        else:
            assert cm.double_bits(got[k]) == cm.double_bits(want[k]), f"compare {what}: {k} {got[k]!r} on the device, {want[k]!r} expected"


def _cmp_map(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, f"compare {what}: map shape"
    COMPARED[0] += got.size
    bad = np.argwhere(cm.bits(got) != cm.bits(want))
    assert len(bad) == 0, (f"compare {what}: map: {len(bad)} values differ, first (y, x, m|r|s) = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} on the device, {want[tuple(bad[0])]!r} expected")


def _cmp_fields(res):
    return tuple(res[k] for k in CMP_INTS) + tuple(cm.double_bits(res[k]) for k in CMP_DOUBLES)


@pytest.mark.parametrize("size", [s for s, _ in sc.COMPARE_SIZES], ids=_ids)
def test_compare_random_pairs_equal_the_model(pt, gpu, size):
    """257 tiles in one row, 257 in one column, 289 and 561 (ragged both ways), strides 14 against 3: the map, the three sums,
    the two counts (both non-zero) and the five doubles."""
    w, h = size
    img, ref, want = sc.compare_random(w, h)
    assert want["saturated"] > 0 and want["nonfinite"] > 0
    got, gmap = pt.compare_frames(img, ref, want_map=True)
    what = f"{w}x{h} ({sc.compare_tiles(w, h)[1]} tiles) random"
    _cmp_result(got, want, what)
    _cmp_map(gmap, cm.stack(want), what)


@pytest.mark.parametrize("size", sc.COMPARE_PLACED_SIZES, ids=_ids)
def test_compare_one_pixel_per_tile(pt, gpu, size):
    """Every tile contributes exactly 2^32 to sum_mse, then exactly one to each count: the sums are the tile count."""
    w, h = size
    tiles = sc.compare_tiles(w, h)[1]
    for name, (img, ref, expect) in (("one pixel per tile", sc.compare_one_pixel_per_tile(w, h)), ("counts per tile", sc.compare_counts_per_tile(w, h))):
        got, gmap = pt.compare_frames(img, ref, want_map=True)
        what = f"{w}x{h} ({tiles} tiles) {name}"
        _cmp_result(got, expect, what + ", constructed", fields=tuple(expect))
        want = cm.compare(img, ref)
        _cmp_result(got, want, what + ", model")
        _cmp_map(gmap, cm.stack(want), what + ", model")


def test_compare_one_tile_per_frame_against_a_shared_reference(pt, gpu):
    """Seven 527 x 263 images in groups of four against one reference, each differing in one pixel of one tile (0, 255, 256, 257,
    511, 512, the last): every sum_mse is 1 << 32 and every m but that pixel's is zero."""
    imgs, ref, lit = sc.compare_one_tile_per_frame()
    n, h, w = imgs.shape[:3]
    px = w * h
    c = pt.Compare(w, h, max_frames=4)
    d_img, d_ref, d_map = pt.DeviceBuffer(imgs.nbytes).upload(imgs), pt.DeviceBuffer(ref.nbytes).upload(ref), pt.DeviceBuffer(n * px * 12)
    try:
        c.run_frames(d_img.ptr, n, d_ref.ptr, d_map.ptr, img_pixel_stride=3, ref_pixel_stride=3, ref_stride_floats=0)
        maps, res = d_map.download(F, (n, h, w, 3)), c.results(n)
    finally:
        c.destroy()
        for d in (d_img, d_ref, d_map):
            d.free()
    for k, t in enumerate(lit):
        what = f"{w}x{h} one pixel in tile {t}, frame {k}"
        x, y = sc.tile_origin(t, w)
        m = np.zeros((h, w), F)
        m[y, x] = 0.25
        _cmp_result(res[k], {"sum_mse": sc.QUARTER, "saturated": 0, "nonfinite": 0, "pixels": px}, what + ", constructed",
                    fields=("sum_mse", "saturated", "nonfinite", "pixels"))
        COMPARED[0] += m.size
        assert np.array_equal(cm.bits(maps[k, ..., 0]), cm.bits(m)), f"compare {what}: map m is not 0.25 at ({x}, {y}) and zero elsewhere"
    for k, t in enumerate(lit):
        what = f"{w}x{h} one pixel in tile {t}, frame {k}"
        want = cm.compare(imgs[k], ref)
        _cmp_result(res[k], want, what + ", model")
        _cmp_map(maps[k], cm.stack(want), what + ", model")


@pytest.mark.parametrize("size", sc.CHECKER_SIZES, ids=_ids)
def test_compare_negative_ssim_sum(pt, gpu, size):
    """A checkerboard against its inverse: every s is negative, so sum_ssim is a negative int64 and ssim a negative double."""
    w, h = size
    img, ref, want = sc.compare_checkerboard(w, h)
    got, gmap = pt.compare_frames(img, ref, want_map=True)
    what = f"{w}x{h} ({sc.compare_tiles(w, h)[1]} tiles) checkerboard"
    assert got["sum_ssim"] < 0 and got["ssim"] < 0.0, f"compare {what}: sum_ssim {got['sum_ssim']}, ssim {got['ssim']!r}: not negative"
    _cmp_result(got, want, what)
    _cmp_map(gmap, cm.stack(want), what)


def test_compare_batch_above_256_tiles_equals_its_singles(pt, gpu):
    """Three 272 x 272 pairs through max_frames 2 (groups of 2 and 1: partials at f * 289), and again after reserve_frames(3) (one
    group), against three single calls and the model; guard bands around the maps and both inputs keep their bytes."""
    imgs, refs, want = sc.compare_batch()
    n, h, w = imgs.shape[:3]
    px = w * h
    singles = [pt.compare_frames(imgs[k], refs[k], want_map=True) for k in range(n)]
    for k in range(n):
        _cmp_result(singles[k][0], want[k], f"{w}x{h} single {k}")
        _cmp_map(singles[k][1], cm.stack(want[k]), f"{w}x{h} single {k}")
    c = pt.Compare(w, h, max_frames=2)
    d_img, d_ref = pt.DeviceBuffer(imgs.nbytes).upload(imgs), pt.DeviceBuffer(refs.nbytes).upload(refs)
    d_map = pt.DeviceBuffer((n * px * 3 + 2 * GUARD) * 4)
    try:
        for turn in ("max_frames 2", "after reserve_frames(3)"):
            pt.check(pt.lib.pt_memset(d_map.ptr, 0x5C, (n * px * 3 + 2 * GUARD) * 4))
            c.run_frames(d_img.ptr, n, d_ref.ptr, d_map.ptr + GUARD * 4, ref_pixel_stride=3)
            raw, res = d_map.download(np.uint32, (n * px * 3 + 2 * GUARD,)), c.results(n)
            assert (raw[:GUARD] == 0x5C5C5C5C).all() and (raw[-GUARD:] == 0x5C5C5C5C).all(), f"compare {w}x{h} batch, {turn}: guard band written"
            maps = raw[GUARD:-GUARD].view(F).reshape(n, h, w, 3)
            for k in range(n):
                what = f"{w}x{h} batch frame {k}, {turn}, against its single"
                _cmp_result(res[k], singles[k][0], what)
                _cmp_map(maps[k], singles[k][1], what)
            c.reserve_frames(3)
        assert c.max_frames == 3
        assert d_img.download(F, imgs.shape).tobytes() == imgs.tobytes(), f"compare {w}x{h} batch: the images were written"
        assert d_ref.download(F, refs.shape).tobytes() == refs.tobytes(), f"compare {w}x{h} batch: the references were written"
    finally:
        c.destroy()
        for d in (d_img, d_ref, d_map):
            d.free()


# ---- training patches --------------------------------------------------------------------------------------------------------

def _pat_values(got, want, what, fields=pm.SUMS + ("values",) + pm.DOUBLES):
    for k in fields:
        COMPARED[0] += 1
        if k in pm.DOUBLES:
            assert pm.double_bits(got[k]) == pm.double_bits(want[k]), f"patches {what}: {k} {got[k]!r} on the device, {want[k]!r} expected"
        else:
            assert got[k] == want[k], f"patches {what}: {k} {got[k]} on the device, {want[k]} expected"


def _pat_tensor(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, f"patches {what}: shape"
    COMPARED[0] += got.size
    bad = np.argwhere(pm.bits(got) != pm.bits(want))
    assert len(bad) == 0, (f"patches {what}: {len(bad)} values differ, first [k][c][j][i] = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} on the device, {want[tuple(bad[0])]!r} expected")


def _pat_against_the_model(s, case, corners, what):
    want, want_in, want_t = sc.patches_model(case, s.p, tuple(corners))
    for k, (g, wv) in enumerate(zip(s.score(corners), want)):
        _pat_values(g, wv, f"{what}, patch {k} at {corners[k]}")
    got_in, got_t = s.gather(corners)  # (asserts that everything outside the n patches kept its bytes)
    _pat_tensor(got_in, want_in, what + ", inputs")
    _pat_tensor(got_t, want_t, what + ", targets")


def test_patches_random_pair_with_258_chunks_equals_the_model(pt, gpu):
    """520 x 516, P = 513, two patches: five trips of max_kernel, 258 partials per patch for sum_kernel (the second patch's at
    258 and up), ten trips of the gather; guard bands and inputs keep their bytes."""
    frame, gt = sc.patches_random()
    s = Rig(pt, frame, gt, sc.BIG_PATCH, len(sc.BIG_CORNERS))
    try:
        s.prepare()
        _pat_against_the_model(s, "random", list(sc.BIG_CORNERS), f"{_ids(sc.PATCH_FRAME)} P={sc.BIG_PATCH} random")
        assert s.inputs_untouched(), f"patches {_ids(sc.PATCH_FRAME)} P={sc.BIG_PATCH}: an input was written"
    finally:
        s.close()


def test_patches_random_pair_small_patches_equal_the_model(pt, gpu):
    """The same frame at P = 8, the stages' ten corners: the divisors come from all five trips and all 256 partial maxima."""
    frame, gt = sc.patches_random()
    corners = sc.small_corners()
    s = Rig(pt, frame, gt, sc.SMALL_PATCH, len(corners))
    try:
        s.prepare()
        _pat_against_the_model(s, "random", corners, f"{_ids(sc.PATCH_FRAME)} P={sc.SMALL_PATCH} random")
    finally:
        s.close()


def test_patches_planted_maxima_reach_the_divisors(pt, gpu):
    """Each of channels 9-13 has its maximum in one pixel that no patch holds: at the start of the second trip, in the last
    pixel, at the end of the first trip (workgroup 255: wave 3 of the gather's fold), in pixel 0 and in the third trip.  The
    gathered channels are the frame's divided by the planted values' divisors."""
    frame, gt, div = sc.patches_planted()
    corners, p = list(sc.PLANTED_CORNERS), sc.SMALL_PATCH
    s = Rig(pt, frame, gt, p, len(corners))
    try:
        s.prepare()
        what = f"{_ids(sc.PATCH_FRAME)} P={p} planted maxima"
        got_in, _ = s.gather(corners)
        for c in range(9, 14):
            with np.errstate(all="ignore"):
                want = np.stack([frame[y:y + p, x:x + p, c] / div[c - 9] for x, y in corners])
            _pat_tensor(np.ascontiguousarray(got_in[:, c]), want, f"{what}: channel {c} (maximum at pixel {sc.PLANTED[c]}), constructed")
        _pat_against_the_model(s, "planted", corners, what + ", model")
    finally:
        s.close()


def test_patches_constant_normal_has_known_sums(pt, gpu):
    """Normal (1, 0, 0), colour 0: the normal's sums are (P^2 2^20, 16 P^2, 0, 0) over 258 chunks, the colour's all zero."""
    frame, gt, sums = sc.patches_constant_normal()
    s = Rig(pt, frame, gt, sc.BIG_PATCH, len(sc.BIG_CORNERS))
    try:
        s.prepare()
        corners = list(sc.BIG_CORNERS)
        want = sc.patches_model("normal", sc.BIG_PATCH, sc.BIG_CORNERS)[0]
        for k, g in enumerate(s.score(corners)):
            what = f"{_ids(sc.PATCH_FRAME)} P={sc.BIG_PATCH} constant normal, patch {k} at {corners[k]}"
            _pat_values(g, sums, what + ", constructed", fields=pm.SUMS)
            _pat_values(g, want[k], what + ", model")
    finally:
        s.close()
