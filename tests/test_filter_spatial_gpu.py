"""The feature filter's spatial variance estimate on the GPU (pt_filter_set_spatial, spatial_kernel in csrc/pt_filter.hip) against
its NumPy restatement (tests/filter_spatial_model.py).

Parity measure and bound are test_filter_gpu.py's: E = max |hip - m64| / (|m64| + 1e-3) <= 16 x E32, E32 the float32 twin's
value of the same measure on the same input -- on the filtered output, and on sqrt(var) right after the set-up (the lab
library's pt_debug_filter_state with no step).  Frames: the three committed 64 x 64 oracle frames and their crops, 9 x 33 and
33 x 9 among them (one column, one row into a second workgroup).  Then: off means off, batches, the CLI."""
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import filter_spatial_model as fsm
from conftest import ROOT
from test_filter_gpu import FACTOR, GOLDEN_FRAMES, _read_exr, bits, golden

pytestmark = pytest.mark.gpu

SHAPES = {"64x64": (slice(0, 64), slice(0, 64)), "29x37": (slice(17, 46), slice(11, 48)), "5x64": (slice(30, 35), slice(0, 64)),
          "64x3": (slice(0, 64), slice(40, 43)), "9x33": (slice(24, 33), slice(13, 46)), "33x9": (slice(13, 46), slice(24, 33)),
          "1x1": (slice(16, 17), slice(59, 60))}  # rows x columns, test_filter_gpu.py's crops and the two 33 / 9 ones
BELOW = 4  # the count images hold BELOW - 1, BELOW and BELOW + 1


def crop(k, shape):
    img, spp = golden(k)
    ys, xs = SHAPES[shape]
    return np.ascontiguousarray(img[ys, xs]), spp


def bound(got, m64, m32, what):
    e, e32 = fm.rel_err(got, m64), fm.rel_err(m32, m64)
    print(f"PARITY {what}: E = {e:.3e}, E32 = {e32:.3e}, E / E32 = {e / e32 if e32 else float('nan'):.2f}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert e <= FACTOR * e32, (what, e, e32)


def straddling_counts(h, w, seed):
    counts = np.random.default_rng(seed).choice(np.array([BELOW - 1, BELOW, BELOW + 1], dtype=np.uint32), (h, w))
    if h * w >= 9:
        assert set(np.unique(counts).tolist()) == {BELOW - 1, BELOW, BELOW + 1}
    return counts


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", [0, 1, 2], ids=["spp1", "spp4", "spp16b8"])
def test_model_parity(pt, lab, gpu, k, shape):
    """R = 1, 2, 3; sqrt(var) after the set-up and the output after 1 and 5 iterations; once with the frame's uniform count and
    below = all, once with a count image that straddles below."""
    frame, spp = crop(k, shape)
    h, w = frame.shape[:2]
    counts = straddling_counts(h, w, 100 + k)
    d_frame = lab.DeviceBuffer(frame.nbytes).upload(frame)
    d_counts = lab.DeviceBuffer(h * w * 4).upload(counts)
    try:
        for radius in (1, 2, 3):
            for name, below, samples, cnt, d_cnt in (("uniform", fsm.ALL, spp, None, None), ("counts", BELOW, 0, counts, d_counts.ptr)):
                what = f"{GOLDEN_FRAMES[k][0]} {shape} R = {radius} {name}"
                ff = lab.FeatureFilter(w, h, spatial_below=below, spatial_radius=radius)
                try:
                    state, _, _ = ff.state(d_frame.ptr, samples, (), d_counts=d_cnt)
                finally:
                    ff.destroy()
                model = dict(samples=samples or None, counts=cnt, below=below, radius=radius)
                _, v64, _, _ = fsm.setup(frame, dtype=np.float64, **model)
                ill32, v32, _, _ = fsm.setup(frame, dtype=np.float32, **model)
                assert np.array_equal(bits(state[..., :3]), bits(ill32)), what  # ill passes through bit for bit
                bound(np.sqrt(state[..., 3].astype(np.float64)), np.sqrt(v64), np.sqrt(v32.astype(np.float64)), what + " sqrt(var)")
                for it in (1, 5):
                    rgb = pt.filter_frame(frame, samples, counts=cnt, iterations=it, spatial_below=below, spatial_radius=radius)[..., :3]
                    bound(rgb, fsm.filter_model(frame, iterations=it, dtype=np.float64, **model),
                          fsm.filter_model(frame, iterations=it, dtype=np.float32, **model), what + f" iterations {it}")
    finally:
        d_frame.free()
        d_counts.free()


# ---- off means off ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["64x64", "29x37", "1x1"])
def test_off_is_the_plain_filter_bit_for_bit(pt, lab, gpu, shape):
    """set_spatial(0), set_spatial(NULL) after it was on, a uniform count at the threshold and a count image with every pixel at
    or above the threshold: the bits of a filter that never heard of the mode, in the output and in the state after the set-up;
    one pixel below the threshold changes them (64 x 64)."""
    frame, spp = crop(1, shape)
    h, w = frame.shape[:2]
    counts = np.random.default_rng(5).integers(BELOW, BELOW + 3, (h, w)).astype(np.uint32)
    plain = pt.filter_frame(frame, spp)
    plain_counts = pt.filter_frame(frame, 0, counts=counts)
    for radius in (1, 2, 3):
        ff = pt.FeatureFilter(w, h, spatial_below="all", spatial_radius=radius)
        try:
            on = pt.filter_frame(frame, spp, filt=ff)
            assert (h * w == 1) == np.array_equal(bits(on), bits(plain))
            ff.set_spatial(0, radius)
            assert np.array_equal(bits(pt.filter_frame(frame, spp, filt=ff)), bits(plain))
            ff.set_spatial("all", radius)
            ff.set_spatial(None)
            assert np.array_equal(bits(pt.filter_frame(frame, spp, filt=ff)), bits(plain))
            ff.set_spatial(spp, radius)      # uniform count == below: nothing qualifies
            assert np.array_equal(bits(pt.filter_frame(frame, spp, filt=ff)), bits(plain))
            ff.set_spatial(BELOW, radius)    # counts all >= below: the kernel runs and hands the state through
            assert np.array_equal(bits(pt.filter_frame(frame, 0, filt=ff, counts=counts)), bits(plain_counts))
            if shape == "64x64":
                low = counts.copy()
                low[20, 20] = BELOW - 1
                assert not np.array_equal(bits(pt.filter_frame(frame, 0, filt=ff, counts=low)), bits(plain_counts))
        finally:
            ff.destroy()
    # the state after the set-up, through the lab library
    d_frame = lab.DeviceBuffer(frame.nbytes).upload(frame)
    d_counts = lab.DeviceBuffer(h * w * 4).upload(counts)
    try:
        ff = lab.FeatureFilter(w, h)
        want = ff.state(d_frame.ptr, 0, (), d_counts=d_counts.ptr)
        ff.set_spatial(BELOW, 3)
        got = ff.state(d_frame.ptr, 0, (), d_counts=d_counts.ptr)
        ff.destroy()
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b))
    finally:
        d_frame.free()
        d_counts.free()


# ---- batches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2, 3])
def test_batches(pt, gpu, radius):
    """Four 64 x 64 frames, strides that leave gaps filled with a sentinel, max_frames 1 and 3: bit for bit four single
    enqueues, out of place and in place (which agree), gaps untouched, twice the same bits; samples >= below launches the
    plain filter for the whole batch."""
    w = h = 64
    spp, n = 2, 4
    frames = [golden(k)[0] for k in range(3)] + [np.ascontiguousarray(golden(1)[0][::-1, ::-1])]
    singles = [pt.filter_frame(f, spp, spatial_below=BELOW, spatial_radius=radius) for f in frames]
    plain = [pt.filter_frame(f, spp) for f in frames]
    assert not any(np.array_equal(bits(a), bits(b)) for a, b in zip(singles, plain))
    fs, rs = w * h * 14 + 37, w * h * 3 + 11
    sentinel = np.float32(-12345.5)
    host = np.full((n, fs), sentinel, np.float32)
    for k, f in enumerate(frames):
        host[k, :w * h * 14] = f.ravel()
    d_frames, d_rgb = pt.DeviceBuffer(host.nbytes), pt.DeviceBuffer(n * rs * 4)
    try:
        for mf in (1, 3):
            ff = pt.FeatureFilter(w, h, max_frames=mf, spatial_below=BELOW, spatial_radius=radius)
            try:
                assert ff.memory() == {"workspace": 64 * w * h * mf, "per_pixel": 64}  # the workspace does not grow
                for _ in range(2):
                    d_frames.upload(host)
                    d_rgb.upload(np.full((n, rs), sentinel, np.float32))
                    ff.enqueue_frames(d_frames.ptr, n, spp, frame_stride_floats=fs, d_rgb=d_rgb.ptr, rgb_stride_floats=rs)
                    pt.check(pt.lib.pt_device_synchronize())
                    rgb = d_rgb.download(np.float32, (n, rs))
                    assert d_frames.download(np.float32, host.shape).tobytes() == host.tobytes()
                    assert (rgb[:, w * h * 3:] == sentinel).all()
                    for k in range(n):
                        assert np.array_equal(bits(rgb[k, :w * h * 3].reshape(h, w, 3)), bits(singles[k][..., :3])), (mf, k)
                ff.run_frames(d_frames.ptr, n, spp, frame_stride_floats=fs)  # in place
                out = d_frames.download(np.float32, host.shape)
                assert (out[:, w * h * 14:] == sentinel).all()
                for k in range(n):
                    assert np.array_equal(bits(out[k, :w * h * 14].reshape(h, w, 14)), bits(singles[k])), (mf, k)
                d_frames.upload(host)
                ff.run_frames(d_frames.ptr, n, BELOW, frame_stride_floats=fs)  # samples == below: no frame qualifies
                out = d_frames.download(np.float32, host.shape)
                for k in range(n):
                    assert np.array_equal(bits(out[k, :w * h * 14].reshape(h, w, 14)), bits(pt.filter_frame(frames[k], BELOW))), (mf, k)
            finally:
                ff.destroy()
        stacked = pt.filter_frames(np.stack(frames), spp, spatial_below=BELOW, spatial_radius=radius)
        assert np.array_equal(bits(stacked), bits(np.stack(singles)))
    finally:
        d_frames.free()
        d_rgb.free()


# ---- the CLI ------------------------------------------------------------------------------------------------------------

def _run(tmp_path, name, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    o = str(tmp_path / name)
    run = subprocess.run([exe, "--size", "64", "-s", "1", "--nobitmap", "-o", o] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    return _read_exr(o + ".exr", 64, 64)


def test_cli_matches_the_python_wrapper(pt, gpu, tmp_path):
    """pathtrace --size 64 -s 1 --filter --filter-spatial-below all: the EXR's colour is what FeatureFilter gives for the
    unfiltered render of the same command, bit for bit (also with --filter-spatial-radius 3), and not the plain filter's."""
    plain = _run(tmp_path, "plain", [])
    for radius, extra in ((2, []), (3, ["--filter-spatial-radius", "3"])):
        got = _run(tmp_path, f"spatial{radius}", ["--filter", "--filter-spatial-below", "all"] + extra)
        want = pt.filter_frame(plain, 1, spatial_below="all", spatial_radius=radius)
        assert np.array_equal(bits(got), bits(want)), radius
    assert not np.array_equal(bits(got), bits(_run(tmp_path, "filtered", ["--filter"])))


def test_cli_with_the_temporal_counts(pt, gpu, tmp_path):
    """--frames 3 --temporal --filter --filter-spatial-below 16 runs (the accumulator's count image reaches the estimate) and
    differs from the run without the option, already at its first frame (--frames 1); below 1 changes nothing."""
    for n in ("1", "3"):
        base = ["--frames", n, "--temporal", "--filter"]
        without = _run(tmp_path, "without" + n, base)
        assert not np.array_equal(bits(_run(tmp_path, "with" + n, base + ["--filter-spatial-below", "16"])), bits(without))
        assert np.array_equal(bits(_run(tmp_path, "one" + n, base + ["--filter-spatial-below", "1"])), bits(without))


def test_cli_with_progressive_and_adaptive_sessions(pt, gpu, tmp_path):
    """--progressive 2 -s 2 --filter --filter-spatial-below 8: the saved frame is FeatureFilter's for the session's frame and
    count (4), bit for bit; under --adaptive the per-pixel counts go in (no pixel stops before 4 samples, so they are all 4 and
    the bits are the same); below 4 leaves the plain filter's bits."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    outs = {}
    for name, extra in (("plain", []), ("filtered", ["--filter"]), ("spatial", ["--filter", "--filter-spatial-below", "8"]),
                        ("at", ["--filter", "--filter-spatial-below", "4"]),
                        ("adaptive", ["--filter", "--filter-spatial-below", "8", "--adaptive", "0.05", "--adaptive-min", "4"])):
        o = str(tmp_path / name)
        run = subprocess.run([exe, "--size", "32", "-s", "2", "--progressive", "2", "--nobitmap", "-o", o] + extra, capture_output=True,
                             text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        outs[name] = _read_exr(o + ".exr", 32, 32)
    assert np.array_equal(bits(outs["spatial"]), bits(pt.filter_frame(outs["plain"], 4, spatial_below=8)))
    assert not np.array_equal(bits(outs["spatial"]), bits(outs["filtered"]))
    assert np.array_equal(bits(outs["at"]), bits(outs["filtered"]))
    assert np.array_equal(bits(outs["adaptive"]), bits(outs["spatial"]))
