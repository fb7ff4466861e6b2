"""The temporal accumulator's NumPy model (tests/temporal_model.py) against expectations that do not come from the definition
(tests/temporal_exact_cases.py): synthetic frames on which every float32 operation is exact, so that plane geometry gives the
output's bits.  Reprojection on frames that are not square, each stop at its threshold and one float beyond it, options and
sample counts the fly-throughs never have, and values that are not finite.  The conditions on the cases themselves are checked
here too, and the host camera step against the dyadic P worked out by hand.  test_temporal_exact_gpu.py holds the kernel to
the same expectations."""
import numpy as np
import pytest

import temporal_exact_cases as tx
import temporal_model as tm


def model(case):
    return tm.run_calls(case.W, case.H, case.calls, **case.opts)


@pytest.mark.parametrize("case", tx.CASES, ids=repr)
def test_model_equals_the_geometric_expectation(case):
    outs, counts = model(case)
    tx.check(case, outs, counts, "model")


@pytest.mark.parametrize("case", tx.NONFINITE, ids=repr)
def test_model_keeps_non_finite_values_where_the_stops_put_them(case):
    """A history pixel that fails a stop contributes nothing, whatever it holds: its weight AND its values are selected away.
    (With the values only multiplied by the 0 weight, NaN and Inf history came out of every pixel whose footprint met it.)"""
    outs, counts = model(case)
    tx.check(case, outs, counts, "model")


@pytest.mark.parametrize("case", tx.CASES + tx.NONFINITE, ids=repr)
def test_the_case_itself_tests_something(case):
    """On the expectation alone: the share of pixels with history is what geometry predicts, the output is not the input,
    the hand-stated pixels are what the expectation says."""
    share = tx.check_inputs(case)
    print(f"{case.name}: {share:.4f} of the pixels with history")


@pytest.mark.parametrize("size", tx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("depth", [8.0, 16.0])
def test_the_eye_shift_moves_the_image_by_the_stated_pixels(size, depth):
    """The construction: from the shifted eye the point of depth z appears (k, j) * 8 / z pixels away, exactly, with the column
    shift divided by H and the row shift by W."""
    W, H = size
    r, c = (a.astype(np.float64) for a in np.mgrid[0:H, 0:W])
    for k, j in tx.shifts(W):
        t, row, col = tx.reproject(W, H, tx.BASIS, tx.EYE, tx.BASIS, tx.shifted_eye(W, H, k, j), np.full((H, W), depth))
        assert np.array_equal(t, np.full((H, W), depth))
        assert np.array_equal(row, r + j * 8.0 / depth) and np.array_equal(col, c + k * 8.0 / depth), (k, j)


def test_camera_step_returns_the_dyadic_matrix_bit_for_bit(pt):
    got, twin = pt.temporal_camera(tx.BASIS), tm.camera_matrix(tx.BASIS)
    assert got.dtype == np.float32 and np.array_equal(got, tx.P_EXACT), got  # the values, worked out by hand
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32))          # and the model's bits (the signs of the zeros)
    # a zero of either sign is the same factor in alpha, beta, gamma: x * (+-0) only meets sums that are not zero
    assert np.array_equal(np.abs(got).view(np.uint32), tx.P_EXACT.view(np.uint32) & np.uint32(0x7FFFFFFF))
