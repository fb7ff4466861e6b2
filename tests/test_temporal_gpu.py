"""The temporal accumulator on the GPU (pt_temporal_*, csrc/pt_temporal.hip) against its float32 NumPy restatement
(tests/temporal_model.py): BIT parity of the frame and of the count image on every frame of a fly-through.  The frames come from
the project's own Renderer (4 spp, generator state carried from frame to frame); no oracle render is needed.  Sizes: 64 x 64 (more
than one workgroup), 37 wide x 29 high (no multiple of the 32 x 8 workgroup), 64 x 3, 3 x 64 and 1 x 1 (every tap at a border)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import temporal_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu

PT_EINVAL = -1
N = 4  # samples per pixel and frame
FRAMES = 6
EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poses(pt, w, h, variant="fly", frames=FRAMES):
    """(bases [K][12], eyes [K][3]) of the fly-through; "turn": the camera turns by 150 degrees at frame 3."""
    bases, eyes = [], []
    for k in range(frames):
        eye, yaw = tm.fly_pose(k)
        if variant == "turn" and k >= 3:
            yaw += 150.0
        eye = tuple(float(np.float32(v)) for v in eye)
        bases.append(pt.camera_basis(eye, yaw=yaw, width=w, height=h))
        eyes.append(eye)
    return np.stack(bases), np.asarray(eyes, dtype=np.float32)


_cache = {}


def sequence(pt, w, h, variant="fly"):
    """The rendered frames of a variant [K][H][W][14] (read-only, rendered once), its cameras and the model's frames and counts."""
    key = (w, h, variant)
    if key not in _cache:
        bases, eyes = poses(pt, w, h, variant)
        spheres = pt.scene_random(40, with_walls=False) if variant == "open" else pt.scene_cornell()
        r = pt.Renderer(w, h, N)
        d_scene, ns = pt.upload_scene(spheres)
        d_out = pt.DeviceBuffer(w * h * 14 * 4)
        try:
            frames = []
            for b, e in zip(bases, eyes):
                r.render(d_out.ptr, d_scene.ptr, ns, b, e)
                frames.append(d_out.download(np.float32, (h, w, 14)))
        finally:
            d_out.free()
            d_scene.free()
            r.destroy()
        frames = np.stack(frames)
        want, want_counts = tm.accumulate_sequence(frames, N, bases, eyes)
        for a in (frames, bases, eyes, want, want_counts):
            a.setflags(write=False)
        _cache[key] = (frames, bases, eyes, want, want_counts)
    return _cache[key]


def run_singles(pt, frames, bases, eyes, session=None, **opts):
    """Every frame through Temporal.run with a count image: (frames after the stage, counts [K][H][W])."""
    k, h, w = frames.shape[:3]
    ta = session or pt.Temporal(w, h, **opts)
    d_frame, d_counts = pt.DeviceBuffer(h * w * 14 * 4), pt.DeviceBuffer(h * w * 4)
    outs, counts = [], []
    try:
        for f, b, e in zip(frames, bases, eyes):
            d_frame.upload(f)
            assert ta.run(d_frame.ptr, N, b, e, d_counts=d_counts.ptr) >= 0
            outs.append(d_frame.download(np.float32, (h, w, 14)))
            counts.append(d_counts.download(np.uint32, (h, w)))
    finally:
        d_frame.free()
        d_counts.free()
        if session is None:
            ta.destroy()
    return np.stack(outs), np.stack(counts)


def assert_bit_parity(got, got_counts, want, want_counts, what):
    for k in range(len(want)):
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, (what, k, len(bad), bad[:5], [(got[k][tuple(i)], want[k][tuple(i)]) for i in bad[:5]])
        assert np.array_equal(got_counts[k], want_counts[k]), (what, k, np.argwhere(got_counts[k] != want_counts[k])[:5])


@pytest.mark.parametrize("size", [(64, 64), (37, 29), (64, 3), (3, 64), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_parity_with_the_model_on_a_fly_through(pt, gpu, size):
    """Share of the pixels of frames 1 .. 5 that find history, measured with the model on these frames: 0.801 .. 0.809 at
    64 x 64 (band 0.5 .. 0.95) and 0.521 .. 0.599 at 37 x 29 (the same margins below and above: 0.22 .. 0.75)."""
    w, h = size
    frames, bases, eyes, want, want_counts = sequence(pt, w, h)
    assert (frames[..., 9] > 0).any()
    if size == (64, 64):  # both branches run: most pixels find history, the rest restart (measured 0.80)
        for k in range(1, FRAMES):
            share = float((want_counts[k] > N).mean())
            print(f"frame {k}: {share:.3f} of the pixels with history")
            assert 0.5 <= share <= 0.95, (k, share)
        assert want_counts.max() == N * FRAMES
    if size == (37, 29):  # the same on the frame that is not square (measured 0.52 .. 0.60; the margins of the 64 x 64 band)
        for k in range(1, FRAMES):
            share = float((want_counts[k] > N).mean())
            print(f"37 x 29 frame {k}: {share:.3f} of the pixels with history")
            assert 0.22 <= share <= 0.75, (k, share)
        assert want_counts.max() == N * FRAMES
    got, got_counts = run_singles(pt, frames, bases, eyes)
    assert_bit_parity(got, got_counts, want, want_counts, size)
    for k in range(FRAMES):  # channels 3-9 and 11-13 untouched
        assert np.array_equal(bits(got[k][..., 3:10]), bits(frames[k][..., 3:10])) and np.array_equal(bits(got[k][..., 11:]), bits(frames[k][..., 11:]))
    if size == (64, 64):
        assert not np.array_equal(bits(got[1:, ..., :3]), bits(frames[1:, ..., :3]))


def test_bit_parity_when_the_camera_turns_away(pt, gpu):
    """150 degrees at frame 3: alpha <= 0 and reprojections outside the frame, nearly every pixel restarts there and
    accumulates again afterwards."""
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64, "turn")
    shares = [float((c > N).mean()) for c in want_counts]
    print("shares with history:", shares)
    assert shares[2] >= 0.5 and shares[3] <= 0.05 and shares[4] >= 0.5
    got, got_counts = run_singles(pt, frames, bases, eyes)
    assert_bit_parity(got, got_counts, want, want_counts, "turn")


def test_bit_parity_in_an_open_scene(pt, gpu):
    """40 spheres without walls: the sky pixels (z <= 0) never accumulate."""
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64, "open")
    sky = frames[..., 9] <= 0
    assert sky.any() and (~sky).any()
    assert (want_counts[sky] == N).all()
    got, got_counts = run_singles(pt, frames, bases, eyes)
    assert_bit_parity(got, got_counts, want, want_counts, "open")


def test_options_reach_the_kernel(pt, gpu):
    """A history cap of 6 samples and other stops: parity with the model given the same options, and other bits than the defaults'."""
    frames, bases, eyes, want_default, _ = sequence(pt, 64, 64)
    opts = dict(history_cap=6.0, depth_tol=0.05, normal_tol=0.5, albedo_tol=0.1, min_weight=0.6)
    want, want_counts = tm.accumulate_sequence(frames, N, bases, eyes, **opts)
    assert want_counts.max() == 10
    got, got_counts = run_singles(pt, frames, bases, eyes, **opts)
    assert_bit_parity(got, got_counts, want, want_counts, "options")
    assert not np.array_equal(bits(want[-1]), bits(want_default[-1]))


def test_reset_passes_the_next_frame_through_and_runs_are_deterministic(pt, gpu):
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64)
    ta = pt.Temporal(64, 64)
    try:
        assert ta.memory() == {"workspace": 96 * 64 * 64, "per_pixel": 96}
        got, got_counts = run_singles(pt, frames[:3], bases[:3], eyes[:3], session=ta)
        assert_bit_parity(got, got_counts, want[:3], want_counts[:3], "before the reset")
        ta.reset()
        got, got_counts = run_singles(pt, frames[3:], bases[3:], eyes[3:], session=ta)
        assert got[0].tobytes() == frames[3].tobytes() and (got_counts[0] == N).all()  # its own bits
        fresh, fresh_counts = tm.accumulate_sequence(frames[3:], N, bases[3:], eyes[3:])
        assert_bit_parity(got, got_counts, fresh, fresh_counts, "after the reset")
        assert (got_counts[1] > N).any()
        ta.reset()
        again, again_counts = run_singles(pt, frames[3:], bases[3:], eyes[3:], session=ta)
        assert np.array_equal(bits(again), bits(got)) and np.array_equal(again_counts, got_counts)
    finally:
        ta.destroy()


def test_frames_form_on_the_renderers_strided_output(pt, gpu):
    """Renderer.enqueue_frames into Temporal.enqueue_frames on one stream, strides that leave gaps filled with a sentinel: the
    bits of single enqueues (and of the model), the last frame's counts, channels 3-9 and 11-13 and the gaps untouched."""
    w, h = 48, 40
    bases, eyes = poses(pt, w, h)
    stride = w * h * 14 + 37
    sentinel = np.float32(-12345.5)
    r = pt.Renderer(w, h, N, variant=6)  # (the variant with a frames kernel)
    ta = pt.Temporal(w, h)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    d_out, d_counts = pt.DeviceBuffer(FRAMES * stride * 4), pt.DeviceBuffer(w * h * 4)
    try:
        d_out.upload(np.full((FRAMES, stride), sentinel, np.float32))
        r.enqueue_frames(d_out.ptr, stride, d_scene.ptr, ns, bases, eyes)
        pt.check(pt.lib.pt_device_synchronize())
        r.check()
        raw = d_out.download(np.float32, (FRAMES, stride))
        ta.enqueue_frames(d_out.ptr, N, bases, eyes, frame_stride_floats=stride, d_counts=d_counts.ptr)
        pt.check(pt.lib.pt_device_synchronize())
        out = d_out.download(np.float32, (FRAMES, stride))
        counts = d_counts.download(np.uint32, (h, w))
    finally:
        for b in (d_out, d_counts, d_scene):
            b.free()
        ta.destroy()
        r.destroy()
    assert (raw[:, w * h * 14:] == sentinel).all() and (out[:, w * h * 14:] == sentinel).all()
    frames = np.ascontiguousarray(raw[:, :w * h * 14]).reshape(FRAMES, h, w, 14)
    got = out[:, :w * h * 14].reshape(FRAMES, h, w, 14)
    assert frames[..., 9].max() > 0
    singles, single_counts = run_singles(pt, frames, bases, eyes)
    assert np.array_equal(bits(got), bits(singles)) and np.array_equal(counts, single_counts[-1])
    assert np.array_equal(bits(got[..., 3:10]), bits(frames[..., 3:10])) and np.array_equal(bits(got[..., 11:]), bits(frames[..., 11:]))
    want, want_counts = tm.accumulate_sequence(frames, N, bases, eyes)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(counts, want_counts[-1])
    assert (want_counts[-1] > N).mean() > 0.5
    # and the host-array helper: one run_frames call
    helped, helped_counts = pt.accumulate_frames(frames, N, bases, eyes)
    assert np.array_equal(bits(helped), bits(singles)) and np.array_equal(helped_counts, single_counts[-1])


def test_static_camera_equals_one_frame_of_all_samples(pt, gpu):
    """Four 4-spp frames of one renderer (persist_rng: the 16 samples of a 16-spp frame) under a camera at rest against the
    GPU's 16-spp frame, with the condition and bounds of the CPU test."""
    size = 64
    basis = pt.camera_basis(width=size, height=size)
    r = pt.Renderer(size, size, N, persist_rng=True)
    ta = pt.Temporal(size, size)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    d_out, d_counts = pt.DeviceBuffer(size * size * 14 * 4), pt.DeviceBuffer(size * size * 4)
    try:
        for _ in range(4):
            r.render(d_out.ptr, d_scene.ptr, ns, basis)
            ta.run(d_out.ptr, N, basis, d_counts=d_counts.ptr)
        acc, counts = d_out.download(np.float32, (size, size, 14)), d_counts.download(np.uint32, (size, size))
    finally:
        for b in (d_out, d_counts, d_scene):
            b.free()
        ta.destroy()
        r.destroy()
    ref, _ = pt.render_frame(size, size, 16, basis=basis)
    tm.static_check(acc, counts, ref, "GPU frames")


def test_composition_with_the_filter(pt, gpu):
    """The accumulator's frame and count image go straight into FeatureFilter.run(d_counts=...): the filter's own measure,
    E <= 16 x E32, against filter_model on the model's output with the model's counts."""
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64)
    w = h = 64
    ta, ff = pt.Temporal(w, h), pt.FeatureFilter(w, h)
    d_frame, d_counts = pt.DeviceBuffer(h * w * 14 * 4), pt.DeviceBuffer(h * w * 4)
    try:
        for f, b, e in zip(frames, bases, eyes):
            d_frame.upload(f)
            ta.enqueue(d_frame.ptr, N, b, e, d_counts=d_counts.ptr)
        ff.run(d_frame.ptr, N, d_counts=d_counts.ptr)
        got = d_frame.download(np.float32, (h, w, 14))
    finally:
        d_frame.free()
        d_counts.free()
        ta.destroy()
        ff.destroy()
    m64 = fm.filter_model(want[-1], counts=want_counts[-1], dtype=np.float64)
    m32 = fm.filter_model(want[-1], counts=want_counts[-1], dtype=np.float32)
    e, e32 = fm.rel_err(got[..., :3], m64), fm.rel_err(m32, m64)
    print(f"COMPOSITION: E = {e:.3e}, E32 = {e32:.3e}, E / E32 = {e / e32:.2f}")
    assert np.isfinite(got).all() and e <= 16.0 * e32
    assert np.array_equal(bits(got[..., 3:]), bits(want[-1][..., 3:]))  # the filter leaves channel 10 as accumulated
    assert fm.rel_err(fm.filter_model(frames[-1], samples=N), m64) > 100 * e  # (and it is not the filter of the plain frame)


def test_invalid_enqueue_arguments_launch_nothing_and_keep_the_session(pt, gpu):
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64)
    w = h = 64
    px = w * h
    fp = ctypes.POINTER(ctypes.c_float)
    ta = pt.Temporal(w, h)
    d_frame = pt.DeviceBuffer(px * 14 * 4)
    try:
        run_singles(pt, frames[:1], bases[:1], eyes[:1], session=ta)
        d_frame.upload(frames[1])
        good_b, good_e = bases[1].ctypes.data_as(fp), eyes[1].ctypes.data_as(fp)
        skew = bases[1].copy()
        skew[9] += 1.0
        nan_eye = np.array([50.0, np.inf, 295.6], np.float32)
        two_b = np.concatenate([bases[1], skew]).astype(np.float32)
        two_e = np.concatenate([eyes[1], eyes[1]]).astype(np.float32)
        L = pt.lib
        calls = [
            (L.pt_temporal_enqueue(ta.handle, None, N, good_b, good_e, None, None), "null d_frame"),
            (L.pt_temporal_enqueue(ta.handle, d_frame.ptr, 0, good_b, good_e, None, None), "samples 0"),
            (L.pt_temporal_run(ta.handle, d_frame.ptr, -2, good_b, good_e, None, None), "samples -2"),
            (L.pt_temporal_enqueue(ta.handle, d_frame.ptr, N, None, good_e, None, None), "null basis"),
            (L.pt_temporal_enqueue(ta.handle, d_frame.ptr, N, good_b, None, None, None), "null eye"),
            (L.pt_temporal_enqueue(ta.handle, d_frame.ptr, N, skew.ctypes.data_as(fp), good_e, None, None), "parallelogram"),
            (L.pt_temporal_run(ta.handle, d_frame.ptr, N, np.zeros(12, np.float32).ctypes.data_as(fp), good_e, None, None), "determinant"),
            (L.pt_temporal_enqueue(ta.handle, d_frame.ptr, N, good_b, nan_eye.ctypes.data_as(fp), None, None), "eye[1]"),
            (L.pt_temporal_enqueue_frames(ta.handle, 0, d_frame.ptr, px * 14, good_b, good_e, N, None, None), "n_frames"),
            (L.pt_temporal_enqueue_frames(ta.handle, 1, None, px * 14, good_b, good_e, N, None, None), "null d_frames"),
            (L.pt_temporal_enqueue_frames(ta.handle, 1, d_frame.ptr, px * 14 - 1, good_b, good_e, N, None, None), "frame_stride_floats"),
            (L.pt_temporal_run_frames(ta.handle, 1, d_frame.ptr, 0, good_b, good_e, N, None, None), "frame_stride_floats"),
            # the SECOND frame's basis is bad: the first is not launched either
            (L.pt_temporal_enqueue_frames(ta.handle, 2, d_frame.ptr, px * 14, two_b.ctypes.data_as(fp), two_e.ctypes.data_as(fp), N, None, None),
             "parallelogram"),
        ]
        for rc, word in calls:
            assert rc == PT_EINVAL, word
        assert L.pt_temporal_enqueue(ta.handle, d_frame.ptr, N, good_b, nan_eye.ctypes.data_as(fp), None, None) == PT_EINVAL
        assert "eye[1]" in L.pt_last_error().decode() and "pt_temporal_enqueue" in L.pt_last_error().decode()
        pt.check(L.pt_device_synchronize())
        assert d_frame.download(np.float32, frames[1].shape).tobytes() == frames[1].tobytes()  # nothing ran on the frame
        # ... and the session is where it was: the next frames continue the sequence
        got, got_counts = run_singles(pt, frames[1:3], bases[1:3], eyes[1:3], session=ta)
        assert_bit_parity(got, got_counts, want[1:3], want_counts[1:3], "after the refused calls")
    finally:
        d_frame.free()
        ta.destroy()


# ---- the CLI --------------------------------------------------------------------------------------------------------

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


def test_cli_accumulates_the_fly_through(pt, gpu, tmp_path):
    """pathtrace --size 64 -s 4 --poses FILE --temporal (six poses): the saved EXR is the model's last frame bit for bit, the
    model fed with the frames a default Renderer produces for the same poses; --temporal-cap reaches the accumulator; with
    --filter the filter receives the accumulator's counts; and without --temporal the saved frame is the plain last render."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    frames, bases, eyes, want, want_counts = sequence(pt, 64, 64)
    pose_file = tmp_path / "poses.txt"
    with open(pose_file, "w") as f:
        for k in range(FRAMES):
            eye, yaw = tm.fly_pose(k)
            f.write(" ".join(repr(float(np.float32(v))) for v in (*eye, yaw, 0.0)) + "\n")
    outs = {}
    for name, extra in (("plain", []), ("temporal", ["--temporal"]), ("cap", ["--temporal", "--temporal-cap", "6"]),
                        ("filtered", ["--temporal", "--filter"])):
        o = str(tmp_path / name)
        run = subprocess.run([exe, "--size", "64", "-s", str(N), "--poses", str(pose_file), "--nobitmap", "-o", o] + extra,
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        assert ("Temporal accumulation completed in" in run.stdout) == bool(extra)
        outs[name] = _read_exr(o + ".exr", 64, 64)
    assert np.array_equal(bits(outs["plain"]), bits(frames[-1]))  # the test renders what the command renders
    assert np.array_equal(bits(outs["temporal"]), bits(want[-1]))
    capped, _ = tm.accumulate_sequence(frames, N, bases, eyes, history_cap=6.0)
    assert np.array_equal(bits(outs["cap"]), bits(capped[-1])) and not np.array_equal(bits(capped[-1]), bits(want[-1]))
    m64 = fm.filter_model(want[-1], counts=want_counts[-1], dtype=np.float64)
    m32 = fm.filter_model(want[-1], counts=want_counts[-1], dtype=np.float32)
    e, e32 = fm.rel_err(outs["filtered"][..., :3], m64), fm.rel_err(m32, m64)
    print(f"CLI --temporal --filter: E = {e:.3e}, E32 = {e32:.3e}")
    assert e <= 16.0 * e32
    assert np.array_equal(bits(outs["filtered"][..., 3:]), bits(want[-1][..., 3:]))


@pytest.mark.parametrize("args,words", [
    (["--temporal", "--progressive", "2"], ["--temporal cannot be combined with --progressive"]),
    (["--temporal", "--batch", "--poses", "none.txt"], ["--temporal cannot be combined with --batch"]),
    (["--temporal"], ["--temporal needs --frames or --poses"]),
    (["--frames", "3", "--temporal-cap", "16"], ["--temporal-cap needs --temporal"]),
    (["--frames", "3", "--temporal", "--temporal-cap", "0.5"], ["--temporal-cap 0.5", ">= 1"]),
    (["--frames", "3", "--temporal", "--temporal-cap", "nan"], ["--temporal-cap", "finite"]),
], ids=["with-progressive", "with-batch", "no-frame-loop", "cap-alone", "cap-below-1", "cap-nan"])
def test_cli_refusals_on_the_built_binary(gpu, tmp_path, args, words):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    run = subprocess.run([exe, "--size", "16"] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr
    assert not os.path.exists(tmp_path / "output")  # nothing was rendered or saved
