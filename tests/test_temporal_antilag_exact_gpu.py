"""The responsive history of the temporal accumulator on the GPU (pt_temporal_set_antilag, pt_temporal_fast; the FAST accumulate
kernel and rectify_kernel<1..3> of csrc/pt_temporal.hip) on the integer-built sequences of temporal_antilag_exact_cases.py:
37 x 19 (partial workgroups on both axes, windows across columns 31 | 32 and rows 7 | 8), 3 x 2 (smaller than the window), 1 x 1 and
64 x 32, each at R = 1, 2, 3.  Every call's 14 channels, counts and fast image against tests/temporal_antilag_model.py bit for bit;
the second call against the expectations stated without the model (below lo, above hi, exactly at lo and hi, sigma = 0, a negative
variance, NaN and Inf in a window, an inactive pixel that is not written, corners and edges with their smaller m, one channel
clamped and two not); the third call shows that the long history received the clamped colour and kept s2."""
import numpy as np
import pytest

import temporal_antilag_exact_cases as ax
import temporal_antilag_model as am

pytestmark = pytest.mark.gpu

f32 = np.float32
_model = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    bad = np.argwhere(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (what, len(bad), bad[:5], [(got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


def model_of(case):
    """The model's (frames, counts, fast images, step-8 records) of a case; computed once, read-only."""
    if case.name not in _model:
        _model[case.name] = am.run_calls(case.W, case.H, case.calls, **case.opts)
    return _model[case.name]


def run_calls(pt, case, opts=None, fast=True):
    """The case's calls through Temporal.run on one session: ([frames], [counts], [fast images])."""
    W, H = case.W, case.H
    ta = pt.Temporal(W, H, **(case.opts if opts is None else opts))
    d_frame, d_counts, d_fast = pt.DeviceBuffer(H * W * 14 * 4), pt.DeviceBuffer(H * W * 4), pt.DeviceBuffer(H * W * 16)
    outs, counts, fasts = [], [], []
    try:
        for F, n, b, e in case.calls:
            assert ta.run(d_frame.upload(F).ptr, n, b, e, d_counts=d_counts.ptr) >= 0
            outs.append(d_frame.download(f32, (H, W, 14)))
            counts.append(d_counts.download(np.uint32, (H, W)))
            if fast:
                assert ta.fast(out=d_fast) is d_fast
                pt.check(pt.lib.pt_device_synchronize())
                fasts.append(d_fast.download(f32, (H, W, 4)))
        assert ta.memory()["per_pixel"] == (128 if fast else 96)
    finally:
        for d in (d_frame, d_counts, d_fast):
            d.free()
        ta.destroy()
    return outs, counts, fasts


@pytest.mark.parametrize("case", ax.CASES, ids=repr)
def test_the_kernels_equal_the_model_and_the_expectation(pt, gpu, case):
    want, want_counts, want_fast, last = model_of(case)
    outs, counts, fasts = run_calls(pt, case)
    for i in range(3):
        assert_same(fasts[i], want_fast[i], (case.name, "fast", i))
        assert_same(outs[i], want[i], (case.name, "frame", i))
        assert np.array_equal(counts[i], want_counts[i]), (case.name, i)
    assert np.array_equal(bits(outs[0]), bits(case.calls[0][0]))  # the first frame passes through: rectify is not issued
    ax.check_second_call(case, outs[1], counts[1], fasts[1], last[1]["x"], "kernel")
    # the third call read a long history that holds the clamped colour and the unclamped s2: its colour and channel 10 say so
    clamped = (last[1]["y"] != last[1]["x"]).any(-1)
    assert clamped.any() or case.W * case.H < 4
    assert_same(outs[2][clamped], want[2][clamped], (case.name, "after the clamp"))


def test_two_runs_give_the_same_bits(pt, gpu):
    case = ax.CASES[1]
    a, b = run_calls(pt, case), run_calls(pt, case)
    for x, y in zip(a[0] + a[2], b[0] + b[2]):
        assert np.array_equal(bits(x), bits(y))
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
