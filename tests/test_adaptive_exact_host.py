"""CPU side of the adaptive stage's exact cases (tests/adaptive_exact_cases.py): the answer each case was CONSTRUCTED to have is
the answer the NumPy model (tests/adaptive_model.py) gives -- set, list, counts, words, block prefix -- so that the GPU file
(tests/test_adaptive_exact_gpu.py) holds the kernels to a construction and to a model that agree.  Plus the assertions on the
constructions themselves: the threshold floats, the M2 search, and the blocks and scan share of every tile size."""
import numpy as np
import pytest

import adaptive_exact_cases as ax
import adaptive_model as am

F32 = np.float32


def model_call(call, what="model"):
    got = am.select(*call.args())
    ax.check_call(call, got, what)
    if not call.peek:
        assert np.array_equal(got[5], call.expect)
    return got


# ---- the constructions -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width, rows, blocks, per", ax.COMPACTION_TILES)
def test_tile_sizes_take_the_scan_paths_the_table_states(width, rows, blocks, per):
    assert ax.blocks_of(width * rows) == blocks and ax.per_of(width * rows) == per
    # one wave of the scan holds 64 lanes' blocks; its 1024 lanes hold one block each up to 1024 blocks
    assert (blocks > 64) == (width * rows > 16384) and (per >= 2) == (width * rows > 262144)


def test_the_scan_paths_are_all_covered():
    blocks = [b for _, _, b, _ in ax.COMPACTION_TILES]
    pers = [p for _, _, _, p in ax.COMPACTION_TILES]
    assert min(blocks) == 1 and any(64 < b <= 1024 for b in blocks) and 1024 in blocks and {1, 2, 3} <= set(pers)
    assert any((w * r) % ax.BLOCK for w, r, _, _ in ax.COMPACTION_TILES)  # a ragged last block


@pytest.mark.parametrize("g", [0.5, 0.125, 1.0, 2.0])
def test_grey_luminance_is_the_grey(g):
    assert ax.lum_of((g, g, g)) == F32(g)
    assert am.luminance(*(np.array([g], F32),) * 3)[0] == F32(g)


@pytest.mark.parametrize("g, tol, n", ax.EXACT_SETTINGS)
def test_exact_thresholds_are_floats_and_m2_is_exact(g, tol, n):
    """Where a power of two sets the scale, T is a float32 itself: the converged variance IS T."""
    assert (n - 1) & (n - 2) == 0
    for floor in (g / 4, g * 4):
        t = ax.threshold(tol, n, g, floor)
        m = max(g, floor)
        assert t == tol * tol * n * m * m and float(F32(t)) == t
        lo, hi = ax.floats_around(t)
        assert float(lo) == t and hi == np.nextafter(lo, F32(np.inf))
        for v in (lo, hi):
            m2 = ax.m2_for(v, n)
            assert float(m2) == float(v) * (n - 1) and F32(m2 / F32(n - 1)) == v


@pytest.mark.parametrize("colour, tol, n", ax.GENERAL_SETTINGS)
def test_general_thresholds_have_an_m2_on_each_side(colour, tol, n):
    lum = ax.lum_of(colour)
    for _, floor in ax._floor_variants(lum):
        t = ax.threshold(tol, n, lum, floor)
        f_lo, f_hi = ax.floats_around(t)
        assert float(f_lo) <= t < float(f_hi) and np.nextafter(f_lo, F32(np.inf)) == f_hi
        (lo, m2_lo), (hi, m2_hi) = ax.variances_around(t, n)
        assert F32(m2_lo / F32(n - 1)) == lo and F32(m2_hi / F32(n - 1)) == hi and float(lo) <= t < float(hi)
        # the floats next to T where a record can hold them (always at n - 1 = 3), else the nearest variance a record can hold
        for want, got in ((f_lo, lo), (f_hi, hi)):
            assert got == want if ax.m2_for(want, n) is not None else abs(int(ax.bits(got)) - int(ax.bits(want))) == 1
        if n == 4:
            assert (lo, hi) == (f_lo, f_hi)


def test_floor_variants_move_the_threshold_by_more_than_a_float():
    """lum one float above the floor and the floor itself give different pairs of floats: a kernel with the wrong m fails one."""
    lum = ax.lum_of((0.25, 0.5, 1.0))
    ts = {name: ax.floats_around(ax.threshold(0.1, 7, lum, floor))[0] for name, floor in ax._floor_variants(lum)}
    assert ts["lum one float below the floor"] > ts["lum one float above the floor"]
    assert ts["lum one float above the floor"] == ts["lum sets T"] and ts["floor sets T"] > ts["lum sets T"]


# ---- every case's constructed answer is the model's ---------------------------------------------------------------------------

@pytest.mark.parametrize("setting", ax.EXACT_SETTINGS + ax.GENERAL_SETTINGS, ids=repr)
def test_model_rule_at_the_threshold(setting):
    colour, tol, n = setting
    for call in ax.rule_threshold_calls(colour, tol, n, exact=np.isscalar(colour)):
        model_call(call)


def test_model_rule_counts_degenerate_values_and_scratch_bits():
    for call in ax.rule_other_calls():
        model_call(call)


@pytest.mark.parametrize("radius", range(5))
@pytest.mark.parametrize("width, rows", ax.DILATION_TILES)
def test_model_dilation(width, rows, radius):
    calls = ax.dilation_calls(width, rows, radius)
    assert len(calls) >= 3
    for call in calls:
        model_call(call)


def test_model_inactive_pixel_is_never_unconverged():
    model_call(ax.inactive_never_unconverged_call())


def test_dilation_windows_do_not_wrap():
    """The case at a row's end: the next row's first pixel is outside the window."""
    calls = [c for c in ax.dilation_calls(37, 29, 2) if "at (14,36)" in c.name and "inactive" not in c.name]
    assert len(calls) == 1
    e = calls[0].expect.reshape(29, 37)
    assert e.sum() == 15 and not e[:, 0].any() and e[12:17, 34:37].all()


@pytest.mark.parametrize("width, rows, blocks, per", ax.COMPACTION_TILES)
def test_model_compaction(width, rows, blocks, per):
    sets = ax.compaction_sets(width * rows)
    assert len(sets) >= (5 if width * rows >= ax.LARGE else 11)
    for name, want in sets.items():
        for mode in (1, 0):
            if mode == 0 and width * rows >= ax.LARGE and name != "random 50%":
                continue
            got = model_call(ax.compaction_call(width, rows, name, want, mode))
            assert np.array_equal(got[2][:int(got[3][0])], np.flatnonzero(want))


def test_model_peek_and_chain():
    want = ax.compaction_sets(1073)["random 50%"]
    for mode in (0, 1):
        peek = ax.compaction_call(37, 29, "random 50%", want, mode, peek=True)
        real = ax.compaction_call(37, 29, "random 50%", want, mode)
        model_call(peek)
        alone = model_call(real)
        assert np.array_equal(alone[0], want)
    state = (np.full(131 * 127, 0xFE, np.uint8), np.zeros(131 * 127, np.uint32), np.full(131 * 127, 0xDEADBEEF, np.uint32), np.array([5, 0], np.uint32))
    for name, rec, n, n_end, mode, peek, expect in ax.chain_steps():
        call = ax.Call(name, rec, 131, n, n_end, mode, peek, 0.5, 0.05, 4, 1, state[0], expect, counts=state[1], lst=state[2], words=state[3])
        got = model_call(call)
        state = got[:4]
    assert state[3].tolist() == [int(expect.sum()), 12] and 0 < expect.sum() < 131 * 127


@pytest.mark.parametrize("pixels", ax.FINALIZE_TILES)
def test_frame_from_record_on_hand_values(pixels):
    """The model's frame on the finalize cases is finite, and on three pixels it is the arithmetic written out."""
    rec, counts = ax.finalize_case(pixels)
    f = am.frame_from_record(rec, counts)
    assert f.shape == (pixels, 14) and np.isfinite(f).all()
    v = rec.view(F32)
    for p in (0, 1, pixels - 1):
        for c in range(10):
            assert f[p, c] == F32(v[c, p] / F32(counts[p]))
        for k in range(4):
            nk = int(rec[10 if k == 0 else 11, p])
            assert f[p, 10 + k] == (F32(v[13 + 2 * k, p] / F32(nk - 1)) if nk >= 2 else 0)
    r = ax.empty_record(2)
    ax.put_pixel(r, 0, (0.25, 0.5, 1.0), 7, var=F32(0.125))
    ax.put_pixel(r, 1, (0.25, 0.5, 1.0), 7, n0=1, m2=F32(3))
    g = am.frame_from_record(r, [7, 7])
    assert g[0, :3].tolist() == [0.25, 0.5, 1.0] and g[0, 10] == F32(0.125) and g[1, 10] == 0 and g[0, 9] == 1


def test_new_symbols_are_lab_only(pt, lab):
    for name in ("pt_debug_adaptive_select", "pt_debug_adaptive_finalize"):
        assert hasattr(lab.lib, name) and not hasattr(pt.lib, name)
    assert callable(lab.debug_adaptive_select) and callable(lab.debug_adaptive_finalize)
