"""The temporal accumulator's kernel (pt_temporal_*, csrc/pt_temporal.hip) on the exact frames of tests/temporal_exact_cases.py:
every case through Temporal.run with a count image, held bit for bit to the expectation worked out from plane geometry AND to
the float32 model (tests/temporal_model.py), channel 10 included.  Reprojection on 64 x 32, 32 x 64 and 16 x 4, each stop at its
threshold and one float beyond, history_cap below the history found, sample counts that change between calls, NaN and Inf in the
history and in the frame; two of the cases again through enqueue_frames with a gapped stride on a stream of their own, and two
sessions of different sizes enqueued alternately.  Frames are at most 64 x 32 and a case is two or three launches."""
import ctypes

import numpy as np
import pytest

import temporal_exact_cases as tx
import temporal_model as tm

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """Equal bits, or NaN on both sides (a NaN that passes through keeps no promised payload)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


_model = {}


def model(case):
    """The model's frames and counts of a case, computed once."""
    if case.name not in _model:
        _model[case.name] = tm.run_calls(case.W, case.H, case.calls, **case.opts)
    return _model[case.name]


def run_case(pt, case):
    """Every call of the case through Temporal.run on one session: ([frame after the stage], [counts])."""
    w, h = case.W, case.H
    ta = pt.Temporal(w, h, **case.opts)
    d_frame, d_counts = pt.DeviceBuffer(h * w * 14 * 4), pt.DeviceBuffer(h * w * 4)
    outs, counts = [], []
    try:
        for F, n, b, e in case.calls:
            d_frame.upload(F)
            assert ta.run(d_frame.ptr, n, b, e, d_counts=d_counts.ptr) >= 0
            outs.append(d_frame.download(np.float32, (h, w, 14)))
            counts.append(d_counts.download(np.uint32, (h, w)))
    finally:
        d_frame.free()
        d_counts.free()
        ta.destroy()
    return outs, counts


def assert_model_parity(case, outs, counts, what):
    want, want_counts = model(case)
    for i in range(len(want)):
        bad = np.argwhere(~same_bits(outs[i], want[i]))
        assert bad.size == 0, (what, case.name, i, len(bad), bad[:5], [(outs[i][tuple(b)], want[i][tuple(b)]) for b in bad[:5]])
        assert np.array_equal(counts[i], want_counts[i]), (what, case.name, i, np.argwhere(counts[i] != want_counts[i])[:5])


@pytest.mark.parametrize("case", tx.CASES, ids=repr)
def test_kernel_equals_the_geometric_expectation_and_the_model(pt, gpu, case):
    outs, counts = run_case(pt, case)
    tx.check(case, outs, counts, "kernel")
    assert_model_parity(case, outs, counts, "kernel")


@pytest.mark.parametrize("case", tx.NONFINITE, ids=repr)
def test_kernel_keeps_non_finite_values_where_the_stops_put_them(pt, gpu, case):
    """A history pixel that fails a stop contributes nothing, whatever it holds; a pixel whose own depth, normal or albedo is NaN
    restarts with its own values and reaches no other pixel, in this call or in the next."""
    outs, counts = run_case(pt, case)
    tx.check(case, outs, counts, "kernel")
    assert_model_parity(case, outs, counts, "kernel")


def _hip_runtime():
    """The HIP runtime the library under test has loaded (the same handle: a library is mapped once)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    hip.hipStreamCreate.argtypes, hip.hipStreamCreate.restype = [ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int
    hip.hipStreamSynchronize.argtypes, hip.hipStreamSynchronize.restype = [ctypes.c_void_p], ctypes.c_int
    hip.hipStreamDestroy.argtypes, hip.hipStreamDestroy.restype = [ctypes.c_void_p], ctypes.c_int
    return hip


@pytest.mark.parametrize("name", tx.STREAMED)
def test_enqueue_frames_on_its_own_stream_with_a_gapped_stride(pt, gpu, name):
    """Both frames of a case in ONE enqueue_frames call on a stream that is not the default one, 37 floats of sentinel behind
    every frame: the expectation's and the model's bits, the last frame's counts, the gaps untouched."""
    case = next(c for c in tx.CASES if c.name == name)
    w, h, k = case.W, case.H, len(case.calls)
    assert all(n == tx.N for _, n, _, _ in case.calls)
    stride = w * h * 14 + 37
    sentinel = np.float32(-12345.5)
    host = np.full((k, stride), sentinel, np.float32)
    for i, (F, _, _, _) in enumerate(case.calls):
        host[i, :w * h * 14] = F.reshape(-1)
    hip = _hip_runtime()
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
    ta = pt.Temporal(w, h, **case.opts)
    d_frames, d_counts = pt.DeviceBuffer(host.nbytes), pt.DeviceBuffer(w * h * 4)
    try:
        d_frames.upload(host)
        ta.enqueue_frames(d_frames.ptr, tx.N, [b for _, _, b, _ in case.calls], [e for _, _, _, e in case.calls],
                          frame_stride_floats=stride, d_counts=d_counts.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        got = d_frames.download(np.float32, (k, stride))
        last_counts = d_counts.download(np.uint32, (h, w))
    finally:
        d_frames.free()
        d_counts.free()
        ta.destroy()
        assert hip.hipStreamDestroy(stream) == 0
    assert (got[:, w * h * 14:] == sentinel).all()
    outs = [np.ascontiguousarray(got[i, :w * h * 14]).reshape(h, w, 14) for i in range(k)]
    counts = [e["counts"] for e in case.expect[:-1]] + [last_counts]  # (only the last frame's counts are written)
    tx.check(case, outs, counts, "enqueue_frames")
    assert_model_parity(case, outs, [c for c in model(case)[1][:-1]] + [last_counts], "enqueue_frames")


def test_two_sessions_of_different_sizes_enqueued_alternately(pt, gpu):
    """64 x 32 and 16 x 4, call by call in turn on the default stream, a device frame per call: each session gives the bits it
    gives alone (and those of the expectation)."""
    cases = [next(c for c in tx.CASES if c.name == n) for n in ("shift-64x32-k-5-j1", "shift-16x4-k0.5-j0")]
    alone = [run_case(pt, c) for c in cases]
    sessions = [pt.Temporal(c.W, c.H, **c.opts) for c in cases]
    frames = [[pt.DeviceBuffer(c.W * c.H * 14 * 4).upload(F) for F, _, _, _ in c.calls] for c in cases]
    counts = [[pt.DeviceBuffer(c.W * c.H * 4) for _ in c.calls] for c in cases]
    try:
        for i in range(2):
            for s, c in enumerate(cases):
                _, n, b, e = c.calls[i]
                sessions[s].enqueue(frames[s][i].ptr, n, b, e, d_counts=counts[s][i].ptr)
        pt.check(pt.lib.pt_device_synchronize())
        for s, c in enumerate(cases):
            outs = [d.download(np.float32, (c.H, c.W, 14)) for d in frames[s]]
            cnts = [d.download(np.uint32, (c.H, c.W)) for d in counts[s]]
            tx.check(c, outs, cnts, "alternating")
            for i in range(2):
                assert same_bits(outs[i], alone[s][0][i]).all() and np.array_equal(cnts[i], alone[s][1][i]), (c.name, i)
    finally:
        for d in [d for per in frames + counts for d in per]:
            d.free()
        for t in sessions:
            t.destroy()
