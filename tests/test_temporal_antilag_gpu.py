"""The responsive history of the temporal accumulator on the GPU (pt_temporal_set_antilag, pt_temporal_fast; csrc/pt_temporal.hip)
on a rendered sequence: the 64 x 64 Cornell box lit by a moving lamp (temporal_antilag_model.lamp_scene), 6 frames at 4 spp from
the project's own Renderer, through the _scene calls with anti-lag on -- every frame's 14 channels, the count image and fast()
after every call against tests/temporal_antilag_model.py bit for bit, the same sequence through enqueue_frames(scenes=) against
the loop, two runs against each other; a session with anti-lag off or never switched on against the plain model, with its
workspace; and the refusals that need a live session."""
import ctypes

import numpy as np
import pytest

import temporal_antilag_model as am
import temporal_motion_model as mm

pytestmark = pytest.mark.gpu

f32 = np.float32
N, SIZE, FRAMES = 4, 64, 6
ANTILAG = dict(fast_cap=8.0)
PT_EINVAL = -1
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    bad = np.argwhere(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (what, len(bad), bad[:5], [(got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


def rendered(pt):
    """The lamp sequence from the project's own Renderer (4 spp, one renderer for the sequence), its scenes [K][9] and cameras;
    rendered once, read-only."""
    if "frames" not in _cache:
        cornell = pt.scene_cornell()
        scenes = np.stack([am.lamp_scene(cornell, k) for k in range(FRAMES)])
        basis = pt.camera_basis(width=SIZE, height=SIZE)
        bases, eyes = np.stack([basis] * FRAMES), np.asarray([pt.DEFAULT_EYE] * FRAMES, f32)
        r = pt.Renderer(SIZE, SIZE, N, rng_mode=pt.RNG_PHILOX)
        d_scene, ns = pt.upload_scene(cornell)
        d_out = pt.DeviceBuffer(SIZE * SIZE * 14 * 4)
        try:
            out = []
            for k in range(FRAMES):
                d_scene.upload(scenes[k])
                r.render(d_out.ptr, d_scene.ptr, ns, basis, pt.DEFAULT_EYE)
                out.append(d_out.download(f32, (SIZE, SIZE, 14)))
        finally:
            d_out.free()
            d_scene.free()
            r.destroy()
        out = np.stack(out)
        for a in (out, scenes, bases, eyes):
            a.setflags(write=False)
        _cache["frames"] = (out, scenes, bases, eyes)
    return _cache["frames"]


def modelled(pt, **opts):
    key = tuple(sorted(opts.items()))
    if key not in _cache:
        frames, scenes, bases, eyes = rendered(pt)
        _cache[key] = am.accumulate_scenes(frames, N, bases, eyes, scenes, **opts)
    return _cache[key]


def fast_image(pt, ta, d_fast):
    """Temporal.fast(out=) into a buffer of the test's own (no torch in this process, as in the motion tests)."""
    assert ta.fast(out=d_fast) is d_fast
    pt.check(pt.lib.pt_device_synchronize())
    return d_fast.download(f32, (SIZE, SIZE, 4))


def single_calls(pt, **opts):
    """The sequence through enqueue(spheres=) and run(spheres=) in turn: (frames, counts, fast images or [], workspace per call)."""
    frames, scenes, bases, eyes = rendered(pt)
    px = SIZE * SIZE
    ta = pt.Temporal(SIZE, SIZE, **opts)
    d_frame, d_counts, d_fast = pt.DeviceBuffer(px * 14 * 4), pt.DeviceBuffer(px * 4), pt.DeviceBuffer(px * 16)
    outs, counts, fasts, memory = [], [], [], []
    try:
        for k in range(FRAMES):
            d_frame.upload(frames[k])
            if k % 2:
                assert ta.run(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scenes[k]) >= 0
            else:
                ta.enqueue(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scenes[k])
                pt.check(pt.lib.pt_device_synchronize())
            outs.append(d_frame.download(f32, (SIZE, SIZE, 14)))
            counts.append(d_counts.download(np.uint32, (SIZE, SIZE)))
            memory.append(ta.memory()["per_pixel"])
            if opts.get("fast_cap", 0.0) > 0:
                fasts.append(fast_image(pt, ta, d_fast))
    finally:
        for d in (d_frame, d_counts, d_fast):
            d.free()
        ta.destroy()
    return np.stack(outs), np.stack(counts), fasts, memory


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_the_lamp_sequence_equals_the_model_frame_by_frame_and_as_one_batch(pt, gpu, radius):
    frames, scenes, bases, eyes = rendered(pt)
    opts = dict(ANTILAG, clamp_sigma=1.5, clamp_radius=radius)
    want, want_counts, want_fast = modelled(pt, **opts)
    plain, _, _ = modelled(pt)
    changed = (bits(want[-1][..., 0:3]) != bits(plain[-1][..., 0:3])).any(-1)
    lamp = mm.first_hit(SIZE, SIZE, scenes[-1], bases[-1], eyes[-1])[2] == am.LAMP_INDEX
    assert changed.mean() > 0.02 and lamp.sum() > 20  # (the clamp acts, and the lamp is in the picture)
    outs, counts, fasts, memory = single_calls(pt, **opts)
    for k in range(FRAMES):
        assert_same(outs[k], want[k], ("single", k))
        assert np.array_equal(counts[k], want_counts[k]), k
        assert_same(fasts[k], want_fast[k], ("fast", k))
    assert memory == [128] + [144] * (FRAMES - 1)  # 96 + 32, and the session's motion image from the second call on
    # all six in ONE enqueue_frames(scenes=) call, 37 floats of sentinel behind every frame
    px = SIZE * SIZE
    stride, sentinel = px * 14 + 37, f32(-12345.5)
    host = np.full((FRAMES, stride), sentinel, f32)
    host[:, :px * 14] = frames.reshape(FRAMES, -1)
    ta = pt.Temporal(SIZE, SIZE, **opts)
    d_frames, d_counts, d_fast = pt.DeviceBuffer(host.nbytes).upload(host), pt.DeviceBuffer(px * 4), pt.DeviceBuffer(px * 16)
    try:
        ta.enqueue_frames(d_frames.ptr, N, bases, eyes, frame_stride_floats=stride, d_counts=d_counts.ptr, scenes=scenes)
        pt.check(pt.lib.pt_device_synchronize())
        got = d_frames.download(f32, (FRAMES, stride))
        assert (got[:, px * 14:] == sentinel).all()
        got = np.ascontiguousarray(got[:, :px * 14]).reshape(frames.shape)
        assert np.array_equal(bits(got), bits(outs))
        assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), counts[-1])
        assert np.array_equal(bits(fast_image(pt, ta, d_fast)), bits(fasts[-1]))
    finally:
        for d in (d_frames, d_counts, d_fast):
            d.free()
        ta.destroy()


def test_the_convenience_passes_the_options_through(pt, gpu):
    frames, scenes, bases, eyes = rendered(pt)
    opts = dict(ANTILAG, clamp_sigma=1.5, clamp_radius=2)
    want, want_counts, _ = modelled(pt, **opts)
    got, last_counts = pt.accumulate_frames(frames, N, bases, eyes, scenes=scenes, **opts)
    assert_same(got, want, "accumulate_frames")
    assert np.array_equal(last_counts, want_counts[-1])


def test_two_runs_of_the_sequence_give_the_same_bits(pt, gpu):
    opts = dict(ANTILAG, clamp_radius=3)
    a, b = single_calls(pt, **opts), single_calls(pt, **opts)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("how", ["never", "fast_cap=0"])
def test_off_is_the_plain_session(pt, gpu, how):
    """A session that never hears of anti-lag, and one told fast_cap = 0: the plain model's bits, 96 bytes per pixel, 112 with the
    motion image.  (On a library without the feature the second form cannot be asked for; the first passes there too.)"""
    frames, scenes, bases, eyes = rendered(pt)
    want, want_counts = mm.accumulate_scenes(frames, N, bases, eyes, scenes)
    px = SIZE * SIZE
    ta = pt.Temporal(SIZE, SIZE)
    d_frame, d_counts = pt.DeviceBuffer(px * 14 * 4), pt.DeviceBuffer(px * 4)
    try:
        if how != "never":
            ta.set_antilag(0.0)
        for k in range(FRAMES):
            ta.run(d_frame.upload(frames[k]).ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scenes[k])
            assert_same(d_frame.download(f32, (SIZE, SIZE, 14)), want[k], (how, k))
            assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), want_counts[k])
            assert ta.memory()["per_pixel"] == (96 if k == 0 else 112)
    finally:
        d_frame.free()
        d_counts.free()
        ta.destroy()


def test_refusals_on_a_live_session_leave_it_as_it_was(pt, gpu):
    """fast_cap >= history_cap, set_antilag after a frame without a reset, fast() with anti-lag off and before a frame, every field
    out of range: PT_EINVAL naming the argument; then the session goes on and gives the model's bits."""
    frames, scenes, bases, eyes = rendered(pt)
    px = SIZE * SIZE
    ta = pt.Temporal(SIZE, SIZE, history_cap=32.0)
    d_frame, d_fast = pt.DeviceBuffer(px * 14 * 4), pt.DeviceBuffer(px * 16)

    def refused(call, *words):
        before = ta.memory()["workspace"]
        with pytest.raises(pt.PtError) as err:
            call()
        assert err.value.code == PT_EINVAL and all(w in str(err.value) for w in words), str(err.value)
        assert ta.memory()["workspace"] == before

    try:
        refused(lambda: ta.fast(out=d_fast), "pt_temporal_fast", "anti-lag is off")
        refused(lambda: ta.set_antilag(32.0), "pt_temporal_set_antilag", "fast_cap")
        refused(lambda: ta.set_antilag(0.5), "fast_cap")
        refused(lambda: ta.set_antilag(float("nan")), "fast_cap")
        refused(lambda: ta.set_antilag(8.0, clamp_sigma=0.0), "clamp_sigma")
        refused(lambda: ta.set_antilag(8.0, clamp_sigma=float("inf")), "clamp_sigma")
        refused(lambda: ta.set_antilag(8.0, clamp_radius=0), "clamp_radius")
        refused(lambda: ta.set_antilag(8.0, clamp_radius=4), "clamp_radius")
        bad = pt.TemporalAntilagOpts(fast_cap=8.0, clamp_sigma=2.0, clamp_radius=2, reserved=1)
        refused(lambda: pt.check(pt.lib.pt_temporal_set_antilag(ta.handle, ctypes.byref(bad))), "reserved")
        refused(lambda: pt.check(pt.lib.pt_temporal_set_antilag(ta.handle, None)), "null opts")
        assert ta.memory()["per_pixel"] == 96
        ta.run(d_frame.upload(frames[0]).ptr, N, bases[0], eyes[0])
        refused(lambda: ta.set_antilag(8.0), "reset the session")
        refused(lambda: ta.fast(out=d_fast), "anti-lag is off")
        ta.reset()
        ta.set_antilag(8.0, clamp_sigma=1.5, clamp_radius=2)
        assert ta.memory()["per_pixel"] == 128
        refused(lambda: ta.fast(out=d_fast), "no frame has run")
        refused(lambda: pt.check(pt.lib.pt_temporal_fast(ta.handle, None, None)), "null d_out")
        model = am.AntilagTemporalModel(SIZE, SIZE, history_cap=32.0, fast_cap=8.0, clamp_sigma=1.5, clamp_radius=2)
        for k in range(3):
            ta.run(d_frame.upload(frames[k]).ptr, N, bases[k], eyes[k], spheres=scenes[k])
            want, _ = model.accumulate_scene(frames[k], N, bases[k], eyes[k], scenes[k])
            assert_same(d_frame.download(f32, (SIZE, SIZE, 14)), want, ("after the refusals", k))
        refused(lambda: ta.set_antilag(0.0), "reset the session")
        # switching off after a reset: today's launches, the buffers stay reported
        ta.reset()
        ta.set_antilag(0.0)
        assert ta.memory()["per_pixel"] == 144
        plain = mm.MotionTemporalModel(SIZE, SIZE, history_cap=32.0)
        for k in range(3):
            ta.run(d_frame.upload(frames[k]).ptr, N, bases[k], eyes[k], spheres=scenes[k])
            want, _ = plain.accumulate_scene(frames[k], N, bases[k], eyes[k], scenes[k])
            assert_same(d_frame.download(f32, (SIZE, SIZE, 14)), want, ("switched off", k))
    finally:
        d_frame.free()
        d_fast.free()
        ta.destroy()
