"""GPU tests of the tone-mapping stage (pt_tonemap_*, csrc/pt_tonemap.hip): bit parity with the float32 NumPy model
(tests/tonemap_model.py) on synthetic frames at ragged sizes, for both strides, every curve, both encodes, metered and fixed
exposure; every sRGB threshold from both sides; the display packer's bytes; adaptation through singles and batches; untouched
input and guard bands; a rendered and filtered frame; the CLI's PPM."""
import os
import subprocess

import numpy as np
import pytest

import tonemap_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu

PT_EINVAL = -1
F = np.float32
CURVES = ["clamp", "reinhard", "aces"]
ENCODES = ["srgb", "linear"]
EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel


def _same_exposure(got, want, what):
    assert tm.scalar_bits(got) == tm.scalar_bits(want), f"{what}: exposure {float(got)!r} (bits {tm.scalar_bits(got):#x}), model {float(want)!r}"


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[0].tolist()}: {got[tuple(bad[0])].tolist()} vs model {want[tuple(bad[0])].tolist()}"


# ---- (a) random frames --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [14, 3])
@pytest.mark.parametrize("size", tm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_frames_equal_the_model(pt, gpu, size, stride):
    """Radiance over 2^-24 .. 2^12 with NaN, +-inf, negatives, zeros and denormals planted: every curve x both encodes x auto
    and two fixed exposures; bytes and exposure bit for bit."""
    w, h = size
    frame = tm.random_frame(w, h, stride, seed=w * 131 + h + stride)
    d_src, d_out = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(w * h * 4)
    try:
        for curve in CURVES:
            for encode in ENCODES:
                for exposure in ("auto", 1.0, 0.037):
                    what = f"{w}x{h} stride {stride} {curve} {encode} exposure {exposure}"
                    t = pt.Tonemap(w, h, curve=curve, encode=encode, exposure=exposure, white=2.5, key=0.22)
                    try:
                        t.run(d_src.ptr, d_out.ptr, pixel_stride=stride)
                        got, e = d_out.download(np.uint8, (h, w, 4)), t.exposure()
                    finally:
                        t.destroy()
                    want, exps = tm.tonemap_sequence([frame], tm.CURVES[curve], tm.ENCODES[encode], 0.0 if exposure == "auto" else exposure,
                                                     key=0.22, white=2.5)
                    _same_exposure(e, exps[0], what)
                    _same_bytes(got, want[0], what)
    finally:
        d_src.free()
        d_out.free()


def test_a_frame_with_nothing_to_meter_keeps_the_exposure(pt, gpu):
    """K = 0: the exposure is 1 with no history, else the previous frame's."""
    w, h = 37, 29
    lit = tm.random_frame(w, h, 3, seed=3)
    dark = np.zeros((h, w, 3), np.float32)
    dark[::2] = np.nan
    dark[1::2, ::3] = -1.0
    t = pt.Tonemap(w, h, adapt=0.5)
    try:
        got = [pt.tonemap_frame(f, tonemap=t) for f in (dark, lit, dark, dark)]
        e = t.exposure()
        want, exps = tm.tonemap_sequence([dark, lit, dark, dark], rate=0.5)
        assert exps[0] == F(1.0) and exps[2] == exps[1]
        _same_exposure(e, exps[3], "dark after lit")
        for k in range(4):
            _same_bytes(got[k], want[k], f"frame {k}")
    finally:
        t.destroy()


# ---- (b) thresholds -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [14, 3])
def test_every_srgb_threshold_from_both_sides(pt, gpu, stride):
    frame = tm.threshold_frame(stride)
    got = pt.tonemap_frame(frame, curve="clamp", encode="srgb", exposure=1.0)
    k = np.arange(1, 256)
    for c in range(3):
        assert np.array_equal(got[2 * c, :, c], k), f"channel {c}: T[k] must encode to k"
        assert np.array_equal(got[2 * c + 1, :, c], k - 1), f"channel {c}: nextafter(T[k], 0) must encode to k - 1"
    _same_bytes(got, tm.map_encode(frame[..., :3], 1.0, tm.CLAMP, tm.SRGB), "threshold frame")


# ---- (c) the display packer ---------------------------------------------------------------------------------------------

def test_clamp_linear_at_exposure_one_equals_the_display_packer(pt, gpu):
    w, h = 300, 70
    frame = tm.random_frame(w, h, 14, seed=11)
    with np.errstate(invalid="ignore"):  # (the planted NaN and inf stay; everything else comes into -1.5 .. 1.5)
        frame[..., :3] = np.where(np.isfinite(frame[..., :3]), np.fmod(frame[..., :3], F(1.5)), frame[..., :3])
    frame[5, :256, 1] = np.nextafter(np.arange(256, dtype=np.float32) / F(255.0), F(0))
    frame[6, :256, 2] = np.arange(256, dtype=np.float32) / F(255.0)
    packed = pt.display_pack(frame)[..., 2].copy().view(np.uint8).reshape(h, w, 4)
    got = pt.tonemap_frame(frame, curve="clamp", encode="linear", exposure=1.0)
    assert np.array_equal(got[..., :3], packed[..., :3]) and (got[..., 3] == 255).all()


# ---- (d) adaptation -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [14, 3])
def test_adaptation_singles_batches_and_model_agree(pt, gpu, stride):
    """Six frames whose brightness steps by x 8, adapt 0.5: singles, one run_frames batch at max_frames 1, 4 and 6 and the model
    agree on every byte and every exposure; after a reset the first frame's exposure is its own target."""
    w, h, n = 37, 29, 6
    frames = tm.stepped_frames(w, h, stride, n)
    want, exps = tm.tonemap_sequence(frames, tm.REINHARD, tm.SRGB, rate=0.5)
    assert len({tm.scalar_bits(e) for e in exps}) == n
    d_src, d_out = pt.DeviceBuffer(frames.nbytes).upload(frames), pt.DeviceBuffer(n * w * h * 4)
    try:
        t = pt.Tonemap(w, h, curve="reinhard", adapt=0.5)
        try:
            for k in range(n):  # singles: the exposure after every frame
                t.run(d_src.ptr + k * frames[0].nbytes, d_out.ptr + k * w * h * 4, pixel_stride=stride)
                _same_exposure(t.exposure(), exps[k], f"single {k}")
            singles = d_out.download(np.uint8, (n, h, w, 4))
            for k in range(n):
                _same_bytes(singles[k], want[k], f"single {k}")
            # after a reset the first frame's exposure is its own target, whatever the session held
            t.reset()
            assert t.exposure() == F(1.0)
            t.run(d_src.ptr + 3 * frames[0].nbytes, d_out.ptr, pixel_stride=stride)
            _same_exposure(t.exposure(), tm.target(*tm.meter(frames[3][..., :3]), 0.18, None), "after reset")
        finally:
            t.destroy()
        for max_frames in (1, 4, 6):
            t = pt.Tonemap(w, h, curve="reinhard", adapt=0.5, max_frames=max_frames)
            try:
                pt.check(pt.lib.pt_memset(d_out.ptr, 0, n * w * h * 4))
                t.run_frames(d_src.ptr, n, d_out.ptr, pixel_stride=stride)
                _same_exposure(t.exposure(), exps[-1], f"batch, max_frames {max_frames}")
                assert d_out.download(np.uint8, (n, h, w, 4)).tobytes() == singles.tobytes(), f"batch, max_frames {max_frames}"
                # the session goes on where the batch ended
                t.run(d_src.ptr, d_out.ptr, pixel_stride=stride)
                _same_exposure(t.exposure(), tm.adapt(exps[-1], tm.target(*tm.meter(frames[0][..., :3]), 0.18, exps[-1]), 0.5),
                               f"after the batch, max_frames {max_frames}")
            finally:
                t.destroy()
    finally:
        d_src.free()
        d_out.free()


def test_batches_with_gaps_and_reserve_frames(pt, gpu):
    """Strides that leave gaps on both sides, a group size grown by reserve_frames (the exposure survives it), fixed exposure."""
    w, h, n, stride = 64, 3, 5, 14
    gap_src, gap_dst = 23, 9
    frames = tm.stepped_frames(w, h, stride, n, seed=8)
    ss, ds = w * h * stride + gap_src, w * h + gap_dst
    src = np.full((n, ss), np.nan, np.float32)
    src[:, :w * h * stride] = frames.reshape(n, -1)
    d_src, d_out = pt.DeviceBuffer(src.nbytes).upload(src), pt.DeviceBuffer(n * ds * 4)
    try:
        for exposure in ("auto", 0.5):
            want, exps = tm.tonemap_sequence(list(frames) + list(frames), tm.ACES, tm.SRGB, 0.0 if exposure == "auto" else exposure, rate=0.25)
            t = pt.Tonemap(w, h, adapt=0.25, exposure=exposure, max_frames=2)
            try:
                small = t.memory()["workspace"]
                for half in range(2):
                    pt.check(pt.lib.pt_memset(d_out.ptr, 0xAB, n * ds * 4))
                    t.run_frames(d_src.ptr, n, d_out.ptr, pixel_stride=stride, src_stride_floats=ss, dst_stride_pixels=ds)
                    out = d_out.download(np.uint8, (n, ds, 4))
                    assert (out[:, w * h:] == 0xAB).all(), "the gaps between the output images are untouched"
                    for k in range(n):
                        _same_bytes(out[k, :w * h].reshape(h, w, 4), want[half * n + k], f"exposure {exposure}, pass {half}, frame {k}")
                    _same_exposure(t.exposure(), exps[half * n + n - 1], f"exposure {exposure}, pass {half}")
                    t.reserve_frames(5)
                assert t.memory()["workspace"] > small and t.max_frames == 5
            finally:
                t.destroy()
    finally:
        d_src.free()
        d_out.free()


# ---- (e) buffers and determinism ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(300, 70), (37, 29), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_untouched_guard_bands_untouched_and_deterministic(pt, gpu, size):
    w, h = size
    guard = 64  # uint32 words on either side of the output
    frame = tm.random_frame(w, h, 14, seed=21)
    d_src, d_out = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer((w * h + 2 * guard) * 4)
    try:
        runs = []
        for _ in range(2):
            pt.check(pt.lib.pt_memset(d_out.ptr, 0x5C, (w * h + 2 * guard) * 4))
            t = pt.Tonemap(w, h)
            try:
                t.run(d_src.ptr, d_out.ptr + guard * 4)
                t.run(d_src.ptr, d_out.ptr + guard * 4)
                runs.append((d_out.download(np.uint32, (w * h + 2 * guard,)), t.exposure()))
            finally:
                t.destroy()
        out, e = runs[0]
        assert (out[:guard] == 0x5C5C5C5C).all() and (out[-guard:] == 0x5C5C5C5C).all(), "guard band written"
        assert (out[guard:-guard] >> 24 == 255).all()
        assert np.array_equal(out, runs[1][0]) and tm.scalar_bits(e) == tm.scalar_bits(runs[1][1]), "two runs differ"
        assert d_src.download(np.float32, frame.shape).tobytes() == frame.tobytes(), "the input was written"
    finally:
        d_src.free()
        d_out.free()


def test_enqueue_refusals_launch_nothing(pt, gpu):
    w, h = 16, 8
    frame = tm.random_frame(w, h, 14, seed=2)
    d_src, d_out = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(w * h * 4)
    t = pt.Tonemap(w, h)
    try:
        pt.check(pt.lib.pt_memset(d_out.ptr, 0x11, w * h * 4))
        for rc, word in [
            (pt.lib.pt_tonemap_enqueue(t.handle, None, 14, d_out.ptr, None), "null d_src"),
            (pt.lib.pt_tonemap_enqueue(t.handle, d_src.ptr, 14, None, None), "null d_rgba8"),
            (pt.lib.pt_tonemap_enqueue(t.handle, d_src.ptr, 2, d_out.ptr, None), "pixel_stride 2"),
            (pt.lib.pt_tonemap_run(t.handle, d_src.ptr, 65, d_out.ptr, None), "pixel_stride 65"),
            (pt.lib.pt_tonemap_enqueue_frames(t.handle, 0, d_src.ptr, w * h * 14, 14, d_out.ptr, w * h, None), "n_frames"),
            (pt.lib.pt_tonemap_enqueue_frames(t.handle, 1, d_src.ptr, w * h * 14 - 1, 14, d_out.ptr, w * h, None), "src_stride_floats"),
            (pt.lib.pt_tonemap_run_frames(t.handle, 1, d_src.ptr, w * h * 14, 14, d_out.ptr, w * h - 1, None), "dst_stride_pixels"),
        ]:
            assert rc == PT_EINVAL, word
        assert pt.lib.pt_tonemap_reserve_frames(t.handle, 1 << 20) == PT_EINVAL and "max_frames" in pt.lib.pt_last_error().decode()
        pt.check(pt.lib.pt_device_synchronize())
        assert (d_out.download(np.uint8, (w * h * 4,)) == 0x11).all()  # nothing ran
        assert t.exposure() == F(1.0)  # and the session is as it was
    finally:
        t.destroy()
        d_src.free()
        d_out.free()


# ---- (f) a rendered frame -----------------------------------------------------------------------------------------------

def test_rendered_and_filtered_frame_equals_the_model(pt, gpu):
    """One 64 x 64 Cornell frame at 4 spp from the project's Renderer, filtered in place, then tone-mapped with the defaults (ACES,
    sRGB, metered); and the out-of-place filter's rgb image (stride 3) gives the same picture."""
    w = h = 64
    frame, _ = pt.render_frame(w, h, 4, basis=pt.camera_basis(width=w, height=h))
    filtered = pt.filter_frame(frame, 4)
    t = pt.Tonemap(w, h)
    try:
        got = pt.tonemap_frame(filtered, tonemap=t)
        e = t.exposure()
    finally:
        t.destroy()
    want, exps = tm.tonemap_sequence([filtered])
    _same_exposure(e, exps[0], "rendered frame")
    _same_bytes(got, want[0], "rendered frame")
    assert 0.05 < float(e) < 20.0 and 20 < got[..., :3].mean() < 235  # a picture, not a flat field
    _, rgb = pt.filter_frame(frame, 4, out_of_place=True)
    _same_bytes(pt.tonemap_frame(rgb), want[0], "stride 3 after the out-of-place filter")


# ---- (g) the CLI --------------------------------------------------------------------------------------------------------

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


def _read_ppm(path, w, h):
    raw = open(path, "rb").read()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
    return np.frombuffer(raw, np.uint8, offset=len(head)).reshape(h, w, 3)


def test_cli_writes_the_tone_mapped_picture(pt, gpu, tmp_path):
    """pathtrace --size 64 -s 4 --filter --tonemap aces: <output>_tm.ppm holds the model's bytes for the saved EXR's colour; the EXR
    is the one the command writes without --tonemap.  Then a fixed exposure with Reinhard and the linear encode."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    base = [exe, "--size", "64", "-s", "4", "--filter", "--nobitmap"]
    plain, mapped, opt = str(tmp_path / "plain"), str(tmp_path / "mapped"), str(tmp_path / "opt")
    for o, extra in ((plain, []), (mapped, ["--tonemap", "aces"]),
                     (opt, ["--tonemap", "reinhard", "--exposure", "0.75", "--tonemap-white", "2", "--tonemap-encode", "linear"])):
        run = subprocess.run(base + ["-o", o] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        assert ("Tone mapping completed in" in run.stdout) == bool(extra)
    assert not os.path.exists(plain + "_tm.ppm")
    assert open(mapped + ".exr", "rb").read() == open(plain + ".exr", "rb").read()
    frame = _read_exr(mapped + ".exr", 64, 64)
    want, exps = tm.tonemap_sequence([frame])
    assert np.array_equal(_read_ppm(mapped + "_tm.ppm", 64, 64), want[0][..., :3])
    want, _ = tm.tonemap_sequence([frame], tm.REINHARD, tm.LINEAR, exposure=0.75, white=2.0)
    assert np.array_equal(_read_ppm(opt + "_tm.ppm", 64, 64), want[0][..., :3])


def test_cli_adapts_through_the_frame_loop(pt, gpu, tmp_path):
    """--frames 3 --tonemap-adapt 0.5: every frame goes through the session, so the picture of the last frame has the exposure
    of three adaptation steps (the frames differ only in their noise, so the steps are small but not zero)."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    o = str(tmp_path / "loop")
    run = subprocess.run([exe, "--size", "32", "-s", "2", "--frames", "3", "--nobitmap", "--tonemap", "clamp", "--tonemap-adapt", "0.5",
                          "-o", o], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = pt.Renderer(32, 32, 2)
    d = pt.DeviceBuffer(32 * 32 * 14 * 4)
    try:
        scene, ns = pt.upload_scene(pt.scene_cornell())
        frames = []
        for _ in range(3):
            r.render(d.ptr, scene.ptr, ns, pt.camera_basis(width=32, height=32))
            frames.append(d.download(np.float32, (32, 32, 14)))
        scene.free()
    finally:
        d.free()
        r.destroy()
    assert np.array_equal(tm.bits(frames[2]), tm.bits(_read_exr(o + ".exr", 32, 32)))
    want, exps = tm.tonemap_sequence(frames, tm.CLAMP, tm.SRGB, rate=0.5)
    assert np.array_equal(_read_ppm(o + "_tm.ppm", 32, 32), want[2][..., :3])
