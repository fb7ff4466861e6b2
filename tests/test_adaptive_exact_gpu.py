"""The adaptive stage's five kernels (csrc/pt_adaptive.hip: classify, decide, scan, scatter, finalize) on the states of
tests/adaptive_exact_cases.py, through the lab library's pt_debug_adaptive_select / pt_debug_adaptive_finalize: no renderer, no
session.  Every call is held bit for bit to the answer its construction gives AND to the NumPy model (tests/adaptive_model.py):
the rule at its threshold and one float beyond, the floor, counts and degenerate values; the dilation's clipped windows on
37 x 29, 1 x 257 and 257 x 1; the list, counts, words and block prefix from 1 pixel to 1024 x 513 (the scan's second wave, every
lane busy, two and three blocks per lane); peek; a chained sequence; the frame of mixed counts in both layouts.  The entry
points put guard words behind every device array and fail the call when one changed.
Sizes: the rule and dilation tiles are at most 1073 pixels; the three largest compaction tiles run a handful of sets each."""
import numpy as np
import pytest

import adaptive_exact_cases as ax
import adaptive_model as am

pytestmark = pytest.mark.gpu

COMPARED = [0]


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    print(f"\ntest_adaptive_exact_gpu: {COMPARED[0]} values compared with their expectation")


def kernel_call(lab, call):
    """The call on the device: against the construction, then every array against the model's."""
    got = lab.debug_adaptive_select(*call.args())
    COMPARED[0] += ax.check_call(call, got, "kernel")
    want = am.select(*call.args())
    names = ("mask", "counts", "list", "words", "block prefix")
    for k, name in enumerate(names):
        a, b = got[k], want[k]
        if k == 0 and call.peek:
            a, b = a & 1, b & 1  # (a peek's scratch bits are its own)
        assert np.array_equal(a, b), (call.name, name, "differs from the model at", np.flatnonzero(np.asarray(a) != np.asarray(b))[:5])
    return got


@pytest.mark.parametrize("setting", ax.EXACT_SETTINGS + ax.GENERAL_SETTINGS, ids=repr)
def test_rule_at_the_threshold(lab, gpu, setting):
    colour, tol, n = setting
    for call in ax.rule_threshold_calls(colour, tol, n, exact=np.isscalar(colour)):
        kernel_call(lab, call)


def test_rule_counts_degenerate_values_and_scratch_bits(lab, gpu):
    for call in ax.rule_other_calls():
        kernel_call(lab, call)


@pytest.mark.parametrize("radius", range(5))
@pytest.mark.parametrize("width, rows", ax.DILATION_TILES)
def test_dilation(lab, gpu, width, rows, radius):
    for call in ax.dilation_calls(width, rows, radius):
        kernel_call(lab, call)


def test_an_inactive_pixel_is_never_unconverged(lab, gpu):
    kernel_call(lab, ax.inactive_never_unconverged_call())


@pytest.mark.parametrize("width, rows, blocks, per", ax.COMPACTION_TILES)
def test_compaction(lab, gpu, width, rows, blocks, per):
    """The forced sets (mode 1) and the same sets made by records (mode 0); on the three largest tiles mode 0 runs one set."""
    for name, want in ax.compaction_sets(width * rows).items():
        for mode in (1, 0):
            if mode == 0 and width * rows >= ax.LARGE and name != "random 50%":
                continue
            kernel_call(lab, ax.compaction_call(width, rows, name, want, mode))


@pytest.mark.parametrize("width, rows", [(1, 1), (37, 29), (131, 127), (513, 512)])
def test_peek_changes_only_its_own_words_and_a_real_call_after_it_is_the_real_call(lab, gpu, width, rows):
    sets = ax.compaction_sets(width * rows)
    for name in ("empty", "random 50%", "only the last pixel"):
        for mode in (1, 0) if width * rows < ax.LARGE else (1,):
            peek = ax.compaction_call(width, rows, name, sets[name], mode, peek=True)
            after_peek = kernel_call(lab, peek)
            real = ax.compaction_call(width, rows, name, sets[name], mode)
            alone = kernel_call(lab, real)
            # the real call on what the peek left (its scratch bits in the mask, its words[0])
            chained = ax.Call(real.name + " after a peek", real.rec, width, real.n, real.n_end, mode, False, real.tol, real.floor,
                              real.min_samples, real.radius, after_peek[0], real.expect, counts=after_peek[1], lst=after_peek[2],
                              words=after_peek[3])
            both = kernel_call(lab, chained)
            for a, b, what in zip(both, alone, ("mask", "counts", "list", "words", "block prefix")):
                assert np.array_equal(a, b), (real.name, what, "differs after a peek")


def test_first_pass_peek_sets_every_pixel(lab, gpu):
    """mode 2 is "every pixel": a peek in that mode reports the whole tile and leaves list, counts and words[1] alone."""
    tp = 1073
    call = ax.Call("37x29 mode 2 peek", ax.empty_record(tp), 37, 0, 4, 2, True, 0.5, 0.05, 2, 1, np.zeros(tp, np.uint8), np.ones(tp, bool))
    kernel_call(lab, call)


def test_chained_sequence(lab, gpu):
    """A first pass, the rule, a peek and the rule again on a shrinking set, each call on the state the one before left."""
    w, rows = 131, 127
    tp = w * rows
    state = (np.full(tp, 0xFE, np.uint8), np.zeros(tp, np.uint32), np.full(tp, 0xDEADBEEF, np.uint32), np.array([5, 0], np.uint32))
    sizes = []
    for name, rec, n, n_end, mode, peek, expect in ax.chain_steps(w, rows, 1):
        call = ax.Call(name, rec, w, n, n_end, mode, peek, 0.5, 0.05, 4, 1, state[0], expect, counts=state[1], lst=state[2], words=state[3])
        got = kernel_call(lab, call)
        state = got[:4]
        sizes.append(int(got[3][0]))
    assert sizes[0] == tp and sizes[1] > sizes[2] == sizes[3] > 0 and state[3][1] == 12
    # the counts tell each pixel's history: 4 (stopped after the first pass), 8, 12
    assert sorted(np.unique(state[1]).tolist()) == [4, 8, 12] and (state[1] == 12).sum() == sizes[3]


def test_refusals_of_the_entry_points(lab, gpu):
    tp = 8
    args = ax.Call("x", ax.empty_record(tp), 4, 4, 5, 1, False, 0.5, 0.05, 2, 0, np.ones(tp, np.uint8), np.ones(tp, bool)).args()
    for k, bad in ((1, 3), (3, 4), (4, 3), (9, 5)):  # width not a divisor, n_end <= n, mode 3, radius 5
        a = list(args)
        a[k] = bad
        with pytest.raises(lab.PtError) as e:
            lab.debug_adaptive_select(*a)
        assert e.value.code == -1


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("pixels", ax.FINALIZE_TILES)
def test_finalize_at_mixed_counts(lab, gpu, pixels, planar):
    rec, counts = ax.finalize_case(pixels)
    want = am.frame_from_record(rec, counts)
    got = lab.debug_adaptive_finalize(rec, counts, planar)
    got = np.ascontiguousarray(got.T) if planar else got
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:5], [(got[tuple(b)], want[tuple(b)], int(counts[b[0]])) for b in bad[:5]])
    COMPARED[0] += got.size
