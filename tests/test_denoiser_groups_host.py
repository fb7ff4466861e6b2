"""CPU side of tests/denoise_group_cases.py (the groups of frames that tests/test_denoiser_groups_gpu.py runs through single
convolutions of the denoiser): from the plan model (tests/denoise_plan_model.py, the rule of csrc/pt_denoise.hip restated, its
constants read from the source) and the float64 reference alone,

  * every reason a case gives for a convolution holds on the model's plan, and over the table, in EACH precision and with more
    than one frame: all five tile shapes, each wide tile with a ragged last tile, each pairing of a wide tile with split-K that
    the rule can produce inside the memory limit, a split lateral, the head split and unsplit (half: unsplit only -- the rule
    cannot split it), a short last K slice;
  * every exactness precondition of the GPU test holds for the seeds and alphabets it uses (asserted inside
    denoise_group_cases.conv_reference): these are conditions, not measurements."""
import numpy as np
import pytest

import denoise_group_cases as GC
import denoise_plan_model as P

PARAMS = GC.params()
IDS = [f"{p}-{w}x{h}-g{g}" for p, w, h, g, _, _ in PARAMS]


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


def test_the_model_reads_the_sources_tables():
    assert P.C["BK"] == 16 and P.C["XC"] == 16 and P.C["kChannels"] == [14, 32, 64, 128, 256, 512, 1024]
    assert set(P.C["kCfg"]) == GC.TILES and len(P.C["kCfg"]) == 5
    for prec in P.PRECISIONS:
        wide, target, min_chunks = P.C["kPlan"][prec]
        assert len(wide) == 3 and target > 0 and min_chunks > 0
    acts, convs = P.layers(37, 29)
    assert len(convs) == 26 and len(acts) == 1 + 18 + 1 + 12
    assert [c["out_hw"] for c in convs if c["name"].endswith("conv2")] == [285, 80, 20, 6, 2, 1]
    assert convs[-1]["out_hw"] == 1073 and convs[-1]["epi"] == P.EPI_RGB


def test_a_group_keeps_the_slicing_and_only_grows_the_tile():
    """batch_plan: the K slicing of one frame is kept, the columns' padding is kept, M = g rows per pixel."""
    for prec in P.PRECISIONS:
        for (w, h, g) in ((37, 29, 816), (100, 75, 32), (512, 512, 32), (1, 1, 300)):
            for one, many in zip(P.plan(w, h, prec, 1), P.plan(w, h, prec, g)):
                assert (many["splits"], many["chunks_per_split"], many["npad"]) == (one["splits"], one["chunks_per_split"], one["npad"])
                assert many["M"] == g * one["M"] and many["npad"] % many["bn"] == 0
                assert many["bm"] * many["bn"] >= one["bm"] * one["bn"], many["name"]
                if many["epi"] != P.EPI_ACT:
                    assert many["bn"] == 32, many["name"]  # launch_conv's condition


@pytest.mark.parametrize("precision,w,h,g,names,reasons", PARAMS, ids=IDS)
def test_every_reason_holds_on_the_models_plan(precision, w, h, g, names, reasons):
    assert g > 1
    rows = GC.rows_of(w, h, precision, g, names)
    assert len(rows) == (26 if names is None else len(names))
    assert GC.failed_reasons(w, h, precision, g, names, reasons) == []
    ws, part = P.workspace_elements(w, h, g, precision)
    assert ws * (2 if precision == "half" else 4) + part * 4 <= GC.MEMORY_LIMIT, (ws, part)


def _covered(precision):
    """{(tile, split?, epilogue, ragged?, short?)} over the table's rows of a precision."""
    out = set()
    for p, w, h, g, names, _ in PARAMS:
        if p == precision:
            for _, c in GC.rows_of(w, h, p, g, names):
                out.add(((c["bm"], c["bn"]), c["splits"] > 1, c["epi"], c["M"] % c["bm"] != 0,
                         c["splits"] > 1 and c["nchunks"] % c["chunks_per_split"] != 0))
    return out


def _largest_group(w, h, precision):
    """The largest group of w x h frames inside the memory and batch limits (both grow with the group)."""
    def fits(g):
        ws, part = P.workspace_elements(w, h, g, precision)
        return g * w * h <= (1 << 26) and ws * (2 if precision == "half" else 4) + part * 4 <= GC.MEMORY_LIMIT

    lo, hi = 1, 65535
    if not fits(1):
        return 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


SEARCH_SIZES = sorted({(w, h) for w, h, *_ in GC.CASES} | {(2, 1), (1, 2), (3, 3), (16, 16), (64, 48), (100, 75), (128, 96), (256, 256),
                                                          (512, 512), (640, 360), (1024, 1024)})


def _producible(precision):
    """{(tile, epilogue)} of the wide-and-split pairings that the rule produces with frames > 1 inside the limits, over
    SEARCH_SIZES.  A tile only grows with the group and the slicing does not depend on it, so the largest group that fits shows
    every pairing of a size."""
    out = {}
    for w, h in SEARCH_SIZES:
        g = _largest_group(w, h, precision)
        if g > 1:
            for c in P.plan(w, h, precision, g):
                if (c["bm"], c["bn"]) in GC.WIDE and c["splits"] > 1:
                    out.setdefault(((c["bm"], c["bn"]), c["epi"]), (w, h, g, c["name"]))
    return out


@pytest.mark.parametrize("precision", P.PRECISIONS)
def test_the_table_covers_every_tile_pairing_and_epilogue_with_frames(precision):
    cov = _covered(precision)
    half = precision == "half"
    assert {t for t, *_ in cov} == GC.TILES
    assert {t for t, _, _, ragged, _ in cov if ragged} >= GC.WIDE, "each wide tile with a ragged last tile"
    assert any(split and epi == P.EPI_LAT for _, split, epi, _, _ in cov), "a split lateral"
    assert any(not split and epi == P.EPI_LAT for _, split, epi, _, _ in cov)
    assert any(not split and epi == P.EPI_RGB for _, split, epi, _, _ in cov), "the head unsplit"
    head = P.plan(37, 29, precision)[-1]
    if half:  # the rule cannot split the half head at any size: its K is a single slice of the least length
        assert head["nchunks"] // P.C["kPlan"]["half"][2] == 1 and not any(split and epi == P.EPI_RGB for _, split, epi, _, _ in cov)
    else:
        assert any(split and epi == P.EPI_RGB for _, split, epi, _, _ in cov), "the head split"
        assert any(t == (256, 32) and split and epi == P.EPI_RGB for t, split, epi, _, _ in cov), "the head split on 256x32"
    assert any(short for *_, short in cov), "a short last K slice"
    can = _producible(precision)
    have = {(t, epi) for t, split, epi, _, _ in cov if split and t in GC.WIDE}
    assert set(can) <= have, {k: v for k, v in can.items() if k not in have}
    want = {((128, 64), P.EPI_ACT), ((128, 128), P.EPI_ACT)} | (set() if half else {((256, 32), P.EPI_ACT), ((256, 32), P.EPI_RGB)})
    assert have == want, have
    assert ((256, 32), P.EPI_LAT) not in can and len(GC.LEFT_OUT) == 1  # the one pairing left out needs more than the limit


def test_the_left_out_pairing_needs_more_than_the_limit():
    """256x32 with split-K under the lateral epilogue: the smallest group of 37 x 29 frames that reaches it, and its memory."""
    first = None
    for g in range(2, 65536, 1):
        c = next(c for c in P.plan(37, 29, "float32", g) if c["name"] == "lat_4")
        if (c["bm"], c["bn"]) == (256, 32):
            first = g
            break
    assert first is not None and 10000 < first < 12000 and c["splits"] > 1, first
    ws, part = P.workspace_elements(37, 29, first, "float32")
    assert ws * 4 + part * 4 > 4 * GC.MEMORY_LIMIT


@pytest.mark.parametrize("precision,w,h,g,names,reasons", PARAMS, ids=IDS)
def test_exactness_preconditions_hold_on_the_reference(dw, precision, w, h, g, names, reasons):
    """The GPU test's inputs (same seeds, same order of draws) through the float64 reference: conv_reference asserts every
    accumulation an integer below 2^24 - 2^12, the float64 affine exact, in half mode every stored affine output an integer of
    magnitude <= 2048 and every lateral reference finite and below 65504.  Every frame's data differs from every other's."""
    half = precision == "half"
    sdi, _ = GC.integer_weights(dw, precision)
    rs = np.random.default_rng(GC.seed_of(w, h, g))
    values = 0
    for _, c in GC.rows_of(w, h, precision, g, names):
        d = GC.conv_inputs(rs, c, g, w, h, half)
        for k in ("x", "res", "up", "x0"):
            if d[k] is not None and d[k][0].size >= 64:
                flat = d[k].reshape(g, -1)
                assert len({f.tobytes() for f in flat[:8]}) == min(g, 8), (c["name"], k)
        for ref in GC.conv_reference(dw, sdi, c, d, half):
            assert ref.shape[0] == g and ref.dtype == np.float32
            values += ref.size
    assert values > 0


def test_the_stacked_reference_is_the_single_frame_reference(dw):
    """conv_ref64_frames is _conv_ref64 (tests/test_denoiser_gpu.py) of each frame."""
    from test_denoiser_gpu import _conv_ref64

    rs = np.random.default_rng(3)
    x = rs.choice(GC.alphabet(False), size=(3, 5, 7, 16))
    wgt = rs.integers(-3, 4, size=(8, 16, 3, 3)).astype(np.float32)
    for stride in (1, 2):
        got = GC.conv_ref64_frames(x, wgt, stride, 3)
        for f in range(3):
            assert np.array_equal(got[f], _conv_ref64(x[f], wgt, stride, 3))
