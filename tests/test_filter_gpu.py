"""The feature-guided filter on the GPU (pt_filter_*, csrc/pt_filter.hip) against its NumPy restatement (tests/filter_model.py).

Parity measure: E = max |hip - m64| / (|m64| + 1e-3) over the output, m64 the float64 model.  Bound: E <= 16 x E32, E32 the
float32 twin's value of the same measure on the same input (about 1e-6); the factor covers the hardware exponential and
another summation order.  Frames: the three committed 64 x 64 oracle frames (1 spp, 4 spp, 16 spp with 8 bounces) and contiguous
crops of them -- 29 rows x 37 columns, 5 x 64, 64 x 3 and 1 x 1 -- the smallest shapes where borders, skipped taps, steps
larger than the frame and the n < 2 rule can go wrong.  No oracle render is needed."""
import functools
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

PT_EINVAL = -1
FACTOR = 16.0
GOLDEN_FRAMES = (("oracle_64_spp1_xorwow", 1), ("oracle_64_spp4_xorwow", 4), ("oracle_64_spp16_xorwow_glm_b8", 16))
SHAPES = {"64x64": (slice(0, 64), slice(0, 64)), "29x37": (slice(17, 46), slice(11, 48)), "5x64": (slice(30, 35), slice(0, 64)),
          "64x3": (slice(0, 64), slice(40, 43)), "1x1": (slice(16, 17), slice(59, 60))}  # (a wall pixel: colour and albedo non-zero and coloured in all three frames)
EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def golden(k):
    name, spp = GOLDEN_FRAMES[k]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert int(z["spp"]) == spp
    img = np.ascontiguousarray(z["image"], dtype=np.float32)
    img.setflags(write=False)
    return img, spp


def crop(k, shape):
    img, spp = golden(k)
    ys, xs = SHAPES[shape]
    return np.ascontiguousarray(img[ys, xs]), spp


def check_parity(got, frame, what, **model_args):
    """E <= 16 x E32 against the float64 model of `frame`; returns E / E32 (printed first)."""
    m64 = fm.filter_model(frame, dtype=np.float64, **model_args)
    m32 = fm.filter_model(frame, dtype=np.float32, **model_args)
    e, e32 = fm.rel_err(got, m64), fm.rel_err(m32, m64)
    print(f"PARITY {what}: E = {e:.3e}, E32 = {e32:.3e}, E / E32 = {e / e32 if e32 else float('nan'):.2f}")
    assert np.isfinite(np.asarray(got)).all()
    assert e <= FACTOR * e32, (what, e, e32)
    return e / e32 if e32 else 0.0


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", [0, 1, 2], ids=["spp1", "spp4", "spp16b8"])
def test_model_parity(pt, gpu, k, shape):
    frame, spp = crop(k, shape)
    assert (frame[..., :3] > 0).any() and (frame[..., 6:9] > 0).any()
    for it in range(1, 6):
        rgb = pt.filter_frame(frame, spp, iterations=it)[..., :3]
        check_parity(rgb, frame, f"{GOLDEN_FRAMES[k][0]} {shape} iterations {it}", samples=spp, iterations=it)


def lane_frame(w, h, n=4):
    """Integers everywhere the filter sums: illumination 0 .. 15 through the unit demodulator a = 2^-8, variance positive
    multiples of 2^-16 / lum(a)^2, depth a ramp (so that dz > 0 wherever depths differ), normals arbitrary."""
    rng = np.random.default_rng(1234 + w)
    f = np.zeros((h, w, 14), np.float32)
    unit = np.float32(2.0 ** -8)
    alb = np.float32(unit - fm.EPS32)
    # the demodulator is exact in both precisions: EPS + albedo is 2^-8, so colour / a and ill x a only move the exponent
    assert np.float32(fm.EPS32 + alb) == unit and np.float64(fm.EPS32) + np.float64(alb) == np.float64(unit)
    f[..., 0:3] = rng.integers(0, 16, (h, w, 3)).astype(np.float32) * unit
    v = rng.normal(size=(h, w, 3))
    f[..., 3:6] = v / np.linalg.norm(v, axis=-1, keepdims=True)
    f[..., 6:9] = alb
    f[..., 9] = 1.0 + np.arange(w)[None, :] + 2.0 * np.arange(h)[:, None]
    f[..., 10] = rng.integers(1, 9, (h, w)).astype(np.float32) * np.float32(n * 2.0 ** -16)
    return f


@pytest.mark.parametrize("size", [(37, 29), (64, 64)], ids=["37x29", "64x64"])
def test_exact_lane_map(lab, gpu, size):
    """All four sigmas 1e30: every exponent is far below 2^-25, exp returns exactly 1, the weights are the dyadic h and every
    sum is exact, so ONE iteration at each step 1, 2, 4, 8, 16 is bit-identical to the float64 model: tap addressing, borders
    and skipped taps.  (The 3 x 3 blur only feeds the luminance stop, which is open here: the parity tests hold it.)"""
    w, h = size
    n = 4
    frame = lane_frame(w, h, n)
    big = dict(sigma_l=1e30, sigma_n=1e30, sigma_a=1e30, sigma_z=1e30)
    ff = lab.FeatureFilter(w, h, **big)
    d_frame, d_rgb = lab.DeviceBuffer(frame.nbytes), lab.DeviceBuffer(h * w * 12)
    try:
        for step in (1, 2, 4, 8, 16):
            m64 = fm.filter_model(frame, samples=n, steps=[step], **big)
            m32 = fm.filter_model(frame, samples=n, steps=[step], dtype=np.float32, **big)
            want = m64.astype(np.float32)
            # exactness on the model side: both precisions agree to the bit (sums exact, quotients correctly rounded), and
            # where all 25 taps are inside (sum of weights 1) the result is the exact dyadic mean, a multiple of 2^-16
            assert np.array_equal(bits(m32), bits(want)), step
            if h > 4 * step and w > 4 * step:
                inner = m64[2 * step:h - 2 * step, 2 * step:w - 2 * step] * 2.0 ** 16
                assert np.array_equal(inner, np.round(inner))
            assert not np.array_equal(want, frame[..., :3])
            d_frame.upload(frame)
            ff.step(d_frame.ptr, n, step, d_rgb=d_rgb.ptr)
            got = d_rgb.download(np.float32, (h, w, 3))
            assert np.array_equal(bits(got), bits(want)), (step, np.argwhere(bits(got) != bits(want))[:5])
            ff.step(d_frame.ptr, n, step)  # in place
            assert np.array_equal(bits(d_frame.download(np.float32, frame.shape)[..., :3]), bits(want)), step
    finally:
        d_frame.free()
        d_rgb.free()
        ff.destroy()


@pytest.mark.parametrize("shape", ["64x64", "29x37"])
def test_in_place_against_out_of_place(pt, gpu, shape):
    frame, spp = crop(1, shape)
    inplace = pt.filter_frame(frame, spp)
    kept, rgb = pt.filter_frame(frame, spp, out_of_place=True)
    assert np.array_equal(bits(inplace[..., :3]), bits(rgb))
    assert np.array_equal(bits(inplace[..., 3:]), bits(frame[..., 3:]))  # channels 3-13 bit for bit as rendered
    assert kept.tobytes() == frame.tobytes()                             # out of place: the frame byte for byte untouched
    assert not np.array_equal(rgb, frame[..., :3])


def test_count_image(pt, gpu):
    """A random per-pixel count image (1 .. 40: the n < 2 rule included) holds the parity bound against the model with the same
    counts; an image of all-equal n gives the bits of samples = n."""
    frame, _ = crop(1, "29x37")
    h, w = frame.shape[:2]
    counts = np.random.default_rng(7).integers(1, 41, (h, w)).astype(np.uint32)
    assert (counts == 1).any()
    got = pt.filter_frame(frame, 0, counts=counts)[..., :3]
    check_parity(got, frame, "29x37 random counts", counts=counts)
    for n in (1, 4):
        same = pt.filter_frame(frame, 0, counts=np.full((h, w), n, np.uint32))
        assert np.array_equal(bits(same), bits(pt.filter_frame(frame, n))), n
    assert not np.array_equal(bits(got), bits(pt.filter_frame(frame, 4)[..., :3]))


def test_batches(pt, gpu):
    """Three 64 x 64 frames, frame and RGB strides that leave gaps filled with a sentinel: bit-identical to three single
    enqueues in place and out of place, gaps untouched, the same bits for max_frames 1, 2 and 3; a reserve_frames that does
    not grow the reservation is a no-op."""
    w = h = 64
    spp = 4
    frames = [golden(k)[0] for k in range(3)]
    singles = [pt.filter_frame(f, spp) for f in frames]
    fs, rs = w * h * 14 + 37, w * h * 3 + 11
    sentinel = np.float32(-12345.5)
    host = np.full((3, fs), sentinel, np.float32)
    for k, f in enumerate(frames):
        host[k, :w * h * 14] = f.ravel()
    d_frames, d_rgb = pt.DeviceBuffer(host.nbytes), pt.DeviceBuffer(3 * rs * 4)
    try:
        for mf in (1, 2, 3):
            ff = pt.FeatureFilter(w, h, max_frames=mf)
            try:
                assert ff.memory() == {"workspace": 64 * w * h * mf, "per_pixel": 64}
                if mf == 3:
                    before = ff.memory()
                    ff.reserve_frames(2)
                    assert ff.memory() == before and ff.max_frames == 3
                # out of place
                d_frames.upload(host)
                d_rgb.upload(np.full((3, rs), sentinel, np.float32))
                ff.enqueue_frames(d_frames.ptr, 3, spp, frame_stride_floats=fs, d_rgb=d_rgb.ptr, rgb_stride_floats=rs)
                pt.check(pt.lib.pt_device_synchronize())
                rgb = d_rgb.download(np.float32, (3, rs))
                assert d_frames.download(np.float32, host.shape).tobytes() == host.tobytes()
                assert (rgb[:, w * h * 3:] == sentinel).all()
                for k in range(3):
                    assert np.array_equal(bits(rgb[k, :w * h * 3].reshape(h, w, 3)), bits(singles[k][..., :3])), (mf, k)
                # in place
                ms = ff.run_frames(d_frames.ptr, 3, spp, frame_stride_floats=fs)
                assert ms > 0
                out = d_frames.download(np.float32, host.shape)
                assert (out[:, w * h * 14:] == sentinel).all()
                for k in range(3):
                    assert np.array_equal(bits(out[k, :w * h * 14].reshape(h, w, 14)), bits(singles[k])), (mf, k)
            finally:
                ff.destroy()
        stacked = pt.filter_frames(np.stack(frames), spp)
        assert np.array_equal(bits(stacked), bits(np.stack(singles)))
    finally:
        d_frames.free()
        d_rgb.free()


def test_straight_from_the_renderer(pt, gpu):
    """Renderer.enqueue_frames into FeatureFilter.enqueue_frames on one stream, the renderer's strided output passed straight
    in: parity against the model on the downloaded unfiltered frames."""
    w, h, spp, n = 48, 40, 4, 3
    bases, eyes = [], []
    for k in range(n):
        eye = (50.0 + 0.7 * k, 52.0 - 0.3 * k, 295.6 - 1.1 * k)
        bases.append(pt.camera_basis(eye, yaw=-90.0 + 0.9 * k, pitch=-0.4 * k, width=w, height=h))
        eyes.append(eye)
    stride = w * h * 14 + 64
    r = pt.Renderer(w, h, spp, variant=6)  # (the variant with a frames kernel: the policy gives so small a tile to variant 8)
    assert r.kernel_info(9)["variant"] == 6
    ff = pt.FeatureFilter(w, h, max_frames=2)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    d_out, d_rgb = pt.DeviceBuffer(n * stride * 4), pt.DeviceBuffer(n * w * h * 12)
    try:
        r.enqueue_frames(d_out.ptr, stride, d_scene.ptr, ns, bases, eyes)
        ff.enqueue_frames(d_out.ptr, n, spp, frame_stride_floats=stride, d_rgb=d_rgb.ptr)
        pt.check(pt.lib.pt_device_synchronize())
        r.check()
        raw = d_out.download(np.float32, (n, stride))
        rgb = d_rgb.download(np.float32, (n, h, w, 3))
        for k in range(n):
            frame = raw[k, :w * h * 14].reshape(h, w, 14)
            assert frame[..., 9].max() > 0
            check_parity(rgb[k], frame, f"renderer frame {k}", samples=spp)
    finally:
        for b in (d_out, d_rgb, d_scene):
            b.free()
        ff.destroy()
        r.destroy()


def test_runs_are_deterministic_and_filters_independent(pt, gpu):
    big, spp = crop(2, "64x64")
    small, _ = crop(2, "29x37")
    a, b = pt.FeatureFilter(64, 64), pt.FeatureFilter(37, 29, iterations=3)
    try:
        a1 = pt.filter_frame(big, spp, filt=a)
        b1 = pt.filter_frame(small, spp, filt=b)
        a2 = pt.filter_frame(big, spp, filt=a)
        b2 = pt.filter_frame(small, spp, filt=b)
    finally:
        a.destroy()
        b.destroy()
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))
    assert np.array_equal(bits(a1), bits(pt.filter_frame(big, spp)))
    assert np.array_equal(bits(b1), bits(pt.filter_frame(small, spp, iterations=3)))


@pytest.mark.parametrize("shape", ["64x64", "29x37", "5x64", "64x3", "1x1"])
def test_tiled_steps_give_the_bits_of_direct_loads(lab, gpu, shape):
    """Steps 1 and 2 through the LDS tile (clamped halo) against direct loads: the same expression on the same values, so the
    same bits, on every shape (borders, a frame smaller than the halo), in place and with a count image."""
    frame, spp = crop(0, shape)
    h, w = frame.shape[:2]
    counts = np.random.default_rng(11).integers(1, 9, (h, w)).astype(np.uint32)
    for it in (1, 2, 5):
        ff = lab.FeatureFilter(w, h, iterations=it)
        try:
            out = {}
            for tiled in (False, True):
                ff.tiled(tiled)
                out[tiled] = (lab.filter_frame(frame, spp, filt=ff), lab.filter_frame(frame, 0, filt=ff, counts=counts))
            assert np.array_equal(bits(out[True][0]), bits(out[False][0])), it
            assert np.array_equal(bits(out[True][1]), bits(out[False][1])), it
            assert np.array_equal(bits(out[False][0]), bits(lab.filter_frame(frame, spp, iterations=it))), it
        finally:
            ff.destroy()


def test_invalid_enqueue_arguments_launch_nothing(pt, gpu):
    w = h = 16
    frame = np.ascontiguousarray(golden(1)[0][:h, :w])
    ff = pt.FeatureFilter(w, h)
    d_frame = pt.DeviceBuffer(frame.nbytes).upload(frame)
    try:
        px = w * h
        calls = [
            (pt.lib.pt_filter_enqueue(ff.handle, None, None, 4, None, None), "d_frame"),
            (pt.lib.pt_filter_enqueue(ff.handle, d_frame.ptr, None, 0, None, None), "samples"),
            (pt.lib.pt_filter_run(ff.handle, d_frame.ptr, None, 0, None, None), "samples"),
            (pt.lib.pt_filter_enqueue_frames(ff.handle, 0, d_frame.ptr, px * 14, None, 0, 4, None), "n_frames"),
            (pt.lib.pt_filter_enqueue_frames(ff.handle, 1, None, px * 14, None, 0, 4, None), "d_frames"),
            (pt.lib.pt_filter_enqueue_frames(ff.handle, 1, d_frame.ptr, px * 14 - 1, None, 0, 4, None), "frame_stride_floats"),
            (pt.lib.pt_filter_enqueue_frames(ff.handle, 1, d_frame.ptr, px * 14, d_frame.ptr, px * 3 - 1, 4, None), "rgb_stride_floats"),
            (pt.lib.pt_filter_run_frames(ff.handle, 1, d_frame.ptr, px * 14, None, 0, -2, None), "samples"),
        ]
        for rc, word in calls:
            assert rc == PT_EINVAL, word
        assert pt.lib.pt_filter_enqueue_frames(ff.handle, 0, d_frame.ptr, px * 14, None, 0, 4, None) == PT_EINVAL
        assert "n_frames" in pt.lib.pt_last_error().decode()
        pt.check(pt.lib.pt_device_synchronize())
        assert d_frame.download(np.float32, frame.shape).tobytes() == frame.tobytes()  # nothing ran on the frame
        with pytest.raises(pt.PtError):
            ff.reserve_frames(1 << 20)
    finally:
        d_frame.free()
        ff.destroy()


def _read_exr(path, w, h):
    raw = open(path, "rb").read()
    block = 8 + w * 14 * 4
    data = raw[len(raw) - h * block:]
    out = np.empty((h, w, 14), np.float32)
    for y in range(h):
        row = np.frombuffer(data, dtype="<f4", count=w * 14, offset=y * block + 8).reshape(14, w)
        for c in range(14):
            out[y, :, EXR_SOURCE[c]] = row[c]
    return out


def test_cli_filters_the_saved_frame(pt, gpu, tmp_path):
    """pathtrace --size 64 -s 4 --filter --nobitmap: the EXR's colour planes hold the parity bound against the model applied to
    the unfiltered render of the same command; the other planes are that render's."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    outs = {}
    for name, extra in (("plain", []), ("filtered", ["--filter"])):
        o = str(tmp_path / name)
        run = subprocess.run([exe, "--size", "64", "-s", "4", "--nobitmap", "-o", o] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        assert ("Filter completed in" in run.stdout) == bool(extra)
        outs[name] = _read_exr(o + ".exr", 64, 64)
    assert np.array_equal(bits(outs["filtered"][..., 3:]), bits(outs["plain"][..., 3:]))
    check_parity(outs["filtered"][..., :3], outs["plain"], "cli 64x64 4 spp", samples=4)
    # and with the options: one iteration, wide stops
    o = str(tmp_path / "opt")
    run = subprocess.run([exe, "--size", "64", "-s", "4", "--nobitmap", "-o", o, "--filter", "--filter-iterations", "2", "--filter-sigma",
                          "8,0.5,0.2,2"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    check_parity(_read_exr(o + ".exr", 64, 64)[..., :3], outs["plain"], "cli options", samples=4, iterations=2, sigma_l=8.0, sigma_n=0.5,
                 sigma_a=0.2, sigma_z=2.0)


def test_cli_filters_progressive_passes(pt, gpu, tmp_path):
    """--progressive 2 -s 2 --filter: the saved frame is the model applied to the session's frame with the session's count (4);
    under --adaptive the per-pixel counts go in (here no pixel stops before 4 samples, so the counts are all 4 as well)."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    base = [exe, "--size", "32", "-s", "2", "--progressive", "2", "--nobitmap"]
    outs = {}
    for name, extra in (("plain", []), ("filtered", ["--filter"]), ("adaptive", ["--filter", "--adaptive", "0.05", "--adaptive-min", "4"])):
        o = str(tmp_path / name)
        run = subprocess.run(base + ["-o", o] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        assert ("Filter completed in" in run.stdout) == bool(extra)
        outs[name] = _read_exr(o + ".exr", 32, 32)
    assert np.array_equal(bits(outs["filtered"][..., 3:]), bits(outs["plain"][..., 3:]))
    check_parity(outs["filtered"][..., :3], outs["plain"], "cli progressive", samples=4)
    assert np.array_equal(bits(outs["adaptive"]), bits(outs["filtered"]))
