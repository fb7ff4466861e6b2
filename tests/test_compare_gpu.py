"""GPU tests of the comparison stage (pt_compare_*, csrc/pt_compare.hip): bit parity with the float32 NumPy model
(tests/compare_model.py) on random HDR frames at sizes that reach every path of the tile kernel, for both pixel strides on either
input; the known answers; batches in groups, with gaps, with one shared reference and after reserve_frames; untouched inputs and
guard bands; refusals that launch nothing; a rendered pair; the CLI's --compare."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import compare_model as cm
import compare_refusal_cases as crc
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel
INTS = ("sum_mse", "sum_relmse", "sum_ssim", "pixels", "saturated", "nonfinite")
DOUBLES = ("mse", "rms", "psnr", "relmse", "ssim")


def _same_result(got, want, what):
    for k in INTS:
        assert got[k] == want[k], f"{what}: {k} {got[k]} on the device, {want[k]} in the model"
    for k in DOUBLES:
        assert cm.double_bits(got[k]) == cm.double_bits(want[k]), f"{what}: {k} {got[k]!r} on the device, {want[k]!r} in the model"


def _same_map(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.argwhere(cm.bits(got) != cm.bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} map values differ, first (y, x, m|r|s) = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} on the device, {want[tuple(bad[0])]!r} in the model")


# ---- (a) random frames --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strides", [(14, 14), (3, 3), (14, 3)], ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("size", cm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_hdr_frames_equal_the_model(pt, gpu, size, strides):
    """Lognormal radiance with NaN, +-inf, negatives, exactly 1.0, 65504 and more planted in both inputs: the map, the three sums,
    the two counts and the derived doubles, bit for bit."""
    w, h = size
    img, ref = cm.hdr_pair(w, h, seed=w * 7 + h, img_stride=strides[0], ref_stride=strides[1])
    want = cm.compare(img, ref)
    if w * h > 1:
        assert want["nonfinite"] > 0 and want["saturated"] > 0 and want["sum_mse"] > 0
    got, gmap = pt.compare_frames(img, ref, want_map=True)
    what = f"{w}x{h} strides {strides}"
    _same_map(gmap, cm.stack(want), what)
    _same_result(got, want, what)


# ---- (b) known answers --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", cm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_images_give_ssim_exactly_one(pt, gpu, size):
    w, h = size
    img, _ = cm.hdr_pair(w, h, seed=w + h, img_stride=14)
    got, gmap = pt.compare_frames(img, img[..., :3], want_map=True)
    assert (cm.bits(gmap[..., 2]) == 0x3F800000).all() and not gmap[..., :2].any()
    assert got["sum_mse"] == 0 and got["sum_relmse"] == 0 and got["sum_ssim"] == (w * h) << 32 and got["saturated"] == 0
    assert (got["mse"], got["rms"], got["psnr"], got["relmse"], got["ssim"]) == (0.0, 0.0, math.inf, 0.0, 1.0)
    assert got["nonfinite"] == cm.compare(img, img)["nonfinite"]


def test_constant_images_have_known_sums(pt, gpu):
    w, h = 37, 29
    got = pt.compare_frames(np.full((h, w, 3), 0.75, F), np.full((h, w, 3), 0.25, F))
    assert got["sum_mse"] == int(w * h * 0.75 * 2 ** 34) and got["mse"] == 0.25 and got["rms"] == 0.5 and got["pixels"] == w * h
    got, gmap = pt.compare_frames(np.full((h, w, 3), 4.0, F), np.zeros((h, w, 3), F), want_map=True)
    assert (gmap[..., 1] == F(3072.0)).all() and got["saturated"] == 3 * w * h and got["relmse"] == 1024.0 and got["nonfinite"] == 0


# ---- (c) batches --------------------------------------------------------------------------------------------------------

def _fields(res):
    return tuple(res[k] for k in INTS) + tuple(cm.double_bits(res[k]) for k in DOUBLES)


def test_batches_in_groups_with_gaps_and_a_shared_reference_equal_the_singles(pt, gpu):
    """Five frames in groups of two (three groups), strides that leave gaps everywhere, then one reference for all five, then the
    same after reserve_frames(5) (one group): every record and every map bit for bit those of five single calls, twice."""
    w, h, n = 37, 29, 5
    px = w * h
    gi, gr, gm = 23, 9, 5  # floats between frames
    pairs = [cm.hdr_pair(w, h, seed=40 + k, img_stride=14, ref_stride=3) for k in range(n)]
    singles = [pt.compare_frames(a, b, want_map=True) for a, b in pairs]
    shared = [pt.compare_frames(a, pairs[0][1], want_map=True) for a, _ in pairs]
    si, sr, sm = px * 14 + gi, px * 3 + gr, px * 3 + gm
    imgs, refs = np.full((n, si), np.nan, F), np.full((n, sr), np.nan, F)
    for k, (a, b) in enumerate(pairs):
        imgs[k, :px * 14], refs[k, :px * 3] = a.ravel(), b.ravel()
    c = pt.Compare(w, h, max_frames=2)
    d_img, d_ref, d_map = pt.DeviceBuffer(imgs.nbytes).upload(imgs), pt.DeviceBuffer(refs.nbytes).upload(refs), pt.DeviceBuffer(n * sm * 4)
    try:
        small = c.memory()["workspace"]
        seen = []
        for turn in range(3):
            for ref_stride, want in ((sr, singles), (0, shared)):
                pt.check(pt.lib.pt_memset(d_map.ptr, 0xAB, n * sm * 4))
                c.run_frames(d_img.ptr, n, d_ref.ptr, d_map.ptr, ref_pixel_stride=3, img_stride_floats=si, ref_stride_floats=ref_stride,
                             map_stride_floats=sm)
                maps = d_map.download(np.uint32, (n, sm))
                assert (maps[:, px * 3:] == 0xABABABAB).all(), "the gaps between the maps are untouched"
                res = c.results(n)
                for k in range(n):
                    what = f"turn {turn}, ref_stride {ref_stride}, frame {k}"
                    assert _fields(res[k]) == _fields(want[k][0]), what
                    _same_map(maps[k, :px * 3].view(np.float32).reshape(h, w, 3), want[k][1], what)
                seen.append((maps.tobytes(), [_fields(r) for r in res]))
            if turn == 1:
                c.reserve_frames(5)
                assert c.memory()["workspace"] > small and c.max_frames == 5
        assert seen[0] == seen[2] == seen[4] and seen[1] == seen[3] == seen[5], "two runs differ"
        assert pt.lib.pt_compare_result(c.handle, n, ctypes.byref(pt.CompareValues())) == crc.PT_EINVAL
        # a single call after a batch: one frame, frame 1 is gone
        c.run(d_img.ptr, d_ref.ptr, None, ref_pixel_stride=3)
        assert _fields(c.result(0)) == _fields(singles[0][0])
        assert pt.lib.pt_compare_result(c.handle, 1, ctypes.byref(pt.CompareValues())) == crc.PT_EINVAL
        assert np.array_equal(d_img.download(np.uint32, imgs.shape), imgs.view(np.uint32)), "the images were written"
        assert np.array_equal(d_ref.download(np.uint32, refs.shape), refs.view(np.uint32)), "the references were written"
    finally:
        c.destroy()
        for d in (d_img, d_ref, d_map):
            d.free()


# ---- (d) side effects ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(300, 70), (17, 15), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_inputs_and_guard_bands_untouched_and_a_null_map_gives_the_same_sums(pt, gpu, size):
    w, h = size
    guard = 64  # floats on either side of the map
    img, ref = cm.hdr_pair(w, h, seed=21, img_stride=14, ref_stride=14)
    c = pt.Compare(w, h)
    d_img, d_ref = pt.DeviceBuffer(img.nbytes).upload(img), pt.DeviceBuffer(ref.nbytes).upload(ref)
    d_map = pt.DeviceBuffer((w * h * 3 + 2 * guard) * 4)
    try:
        pt.check(pt.lib.pt_memset(d_map.ptr, 0x5C, (w * h * 3 + 2 * guard) * 4))
        c.run(d_img.ptr, d_ref.ptr, d_map.ptr + guard * 4)
        with_map = c.result()
        out = d_map.download(np.uint32, (w * h * 3 + 2 * guard,))
        assert (out[:guard] == 0x5C5C5C5C).all() and (out[-guard:] == 0x5C5C5C5C).all(), "guard band written"
        c.run(d_img.ptr, d_ref.ptr, None)
        assert _fields(c.result()) == _fields(with_map), "a NULL d_map changes the sums"
        assert np.array_equal(d_map.download(np.uint32, out.shape), out), "a NULL d_map wrote the old map"
        _same_result(with_map, cm.compare(img, ref), f"{w}x{h}")
        assert d_img.download(np.float32, img.shape).tobytes() == img.tobytes(), "the image was written"
        assert d_ref.download(np.float32, ref.shape).tobytes() == ref.tobytes(), "the reference was written"
    finally:
        c.destroy()
        for d in (d_img, d_ref, d_map):
            d.free()


def test_live_refusals_launch_nothing_and_keep_the_results(pt, gpu):
    """Every refusal of a live 8 x 8 session (tests/compare_refusal_cases.py): PT_EINVAL naming the argument, the map buffer keeps
    its bytes and the two records of the call before are what they were."""
    n, px = 2, crc.PIXELS
    rng = np.random.default_rng(9)
    frames = np.exp(rng.normal(-1.0, 2.0, (2, n, px * 64))).astype(F)
    c = pt.Compare(crc.W, crc.H, max_frames=2)
    d_img, d_ref = pt.DeviceBuffer(frames[0].nbytes).upload(frames[0]), pt.DeviceBuffer(frames[1].nbytes).upload(frames[1])
    d_map = pt.DeviceBuffer(n * px * 3 * 4)
    try:
        values = pt.CompareValues()
        assert pt.lib.pt_compare_result(c.handle, 0, ctypes.byref(values)) == crc.PT_EINVAL  # nothing has been compared yet
        assert "frame_index" in pt.lib.pt_last_error().decode()
        c.run_frames(d_img.ptr, n, d_ref.ptr, None, img_stride_floats=px * 64, ref_stride_floats=px * 64)
        before = [_fields(r) for r in c.results(n)]
        assert before[0] != before[1]
        pt.check(pt.lib.pt_memset(d_map.ptr, 0x11, n * px * 3 * 4))
        cases = crc.live_cases(pt, c.handle, d_img.ptr, d_ref.ptr, d_map.ptr)
        assert crc.play(pt, cases) == len(cases) >= 35
        pt.check(pt.lib.pt_device_synchronize())
        assert (d_map.download(np.uint8, (n * px * 3 * 4,)) == 0x11).all(), "a refused call wrote the map"
        assert [_fields(r) for r in c.results(n)] == before, "a refused call changed the results"
    finally:
        c.destroy()
        for d in (d_img, d_ref, d_map):
            d.free()


# ---- (e) a rendered pair ------------------------------------------------------------------------------------------------

def test_rendered_pair_equals_the_model_and_the_filter_brings_it_closer(pt, gpu):
    """64 x 64 Cornell at 2 spp against 64 spp from the project's Renderer: the device's result is the model's on the downloaded
    frames; the same 2-spp frame after the feature-guided filter has a smaller rms and a larger ssim (a direction, not a bound)."""
    w = h = 64
    basis = pt.camera_basis(width=w, height=h)
    noisy, _ = pt.render_frame(w, h, 2, basis=basis)
    clean, _ = pt.render_frame(w, h, 64, basis=basis)
    got, gmap = pt.compare_frames(noisy, clean, want_map=True)
    want = cm.compare(noisy, clean)
    _same_map(gmap, cm.stack(want), "rendered pair")
    _same_result(got, want, "rendered pair")
    assert 0.01 < got["rms"] < 0.5 and 0.0 < got["ssim"] < 0.9 and got["nonfinite"] == 0
    filtered = pt.compare_frames(pt.filter_frame(noisy, 2), clean)
    assert filtered["rms"] < got["rms"] and filtered["ssim"] > got["ssim"], (filtered, got)


# ---- (f) the CLI --------------------------------------------------------------------------------------------------------

LINE = re.compile(r"^compare: rms (\S+) psnr (\S+) relmse (\S+) ssim (\S+) \(saturated (\d+), nonfinite (\d+)\)$", re.M)


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


def _cli(*args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe, "--nobitmap"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_compares_every_frame_with_the_reference_file(pt, gpu, tmp_path):
    a, b, p = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "p")
    run = _cli("--size", 64, "-s", 4, "-o", a)
    assert run.returncode == 0 and "compare:" not in run.stdout, run.stderr
    # the same frame again: no error at all
    run = _cli("--size", 64, "-s", 4, "-o", b, "--compare", a + ".exr")
    assert run.returncode == 0, run.stderr
    lines = LINE.findall(run.stdout)
    assert len(lines) == 1 and lines[0] == ("0", "inf", "0", "1", "0", "0") and "Comparison completed in" in run.stdout
    assert open(b + ".exr", "rb").read() == open(a + ".exr", "rb").read()  # (the frame keeps its bytes)
    # another sample count: the values compare_frames gives for the two files' colours
    run = _cli("--size", 64, "-s", 8, "-o", b, "--compare", a + ".exr")
    assert run.returncode == 0, run.stderr
    lines = LINE.findall(run.stdout)
    want = pt.compare_frames(_read_exr(b + ".exr", 64, 64), _read_exr(a + ".exr", 64, 64))
    assert len(lines) == 1
    assert [float(v) for v in lines[0][:4]] == [want["rms"], want["psnr"], want["relmse"], want["ssim"]] and want["rms"] > 0
    assert (int(lines[0][4]), int(lines[0][5])) == (want["saturated"], want["nonfinite"])
    # a progressive session: one line per pass, the last one for the saved frame
    run = _cli("--size", 64, "-s", 4, "--progressive", 3, "-o", p, "--compare", a + ".exr")
    assert run.returncode == 0, run.stderr
    lines = LINE.findall(run.stdout)
    want = pt.compare_frames(_read_exr(p + ".exr", 64, 64), _read_exr(a + ".exr", 64, 64))
    assert len(lines) == 3 and float(lines[2][0]) == want["rms"] and float(lines[2][3]) == want["ssim"]


def test_cli_refuses_before_it_renders(pt, gpu, tmp_path):
    a, o = str(tmp_path / "a"), str(tmp_path / "o")
    assert _cli("--size", 32, "-s", 2, "-o", a).returncode == 0
    poses = tmp_path / "poses.txt"
    poses.write_text("50 52 295.6 -90 0\n")
    for args, word in ((["--size", 32, "--poses", poses, "--batch", "--compare", a + ".exr"], "--batch"),
                       (["--size", 32, "--compare", str(tmp_path / "missing.exr")], "missing.exr"),
                       (["--size", 64, "--compare", a + ".exr"], "32 x 32"),
                       (["--size", 32, "--compare", poses], "not an EXR file")):
        run = _cli("-o", o, *args)
        assert run.returncode != 0 and word in run.stderr and "--compare" in run.stderr, (args, run.stderr)
        assert "Render completed" not in run.stdout and not os.path.exists(o + ".exr"), args
