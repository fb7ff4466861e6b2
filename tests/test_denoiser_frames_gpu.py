"""Batches of frames through the denoising network (pt_denoiser_enqueue_frames, csrc/pt_denoise.hip): bit for bit the loop of
single enqueues, in place and out of place, with strides, in groups, straight from pt_renderer_enqueue_frames, and in the
launches of ONE frame per group (the lab getters show the batch path ran, not a loop over frames)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PT_EINVAL = -1


@pytest.fixture(scope="module")
def sd(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights.random_state_dict(seed=5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poses(pt, n, w, h):
    bases, eyes = [], []
    for k in range(n):
        eye = (50.0 + 0.7 * k, 52.0 - 0.3 * k, 295.6 - 1.1 * k)
        bases.append(pt.camera_basis(eye, yaw=-90.0 + 0.9 * k, pitch=-0.4 * k, width=w, height=h))
        eyes.append(eye)
    return np.asarray(bases, dtype=np.float32), np.asarray(eyes, dtype=np.float32)


_base = {}


def make_frames(pt, w, h, n):
    """n different [H][W][14] frames: four poses at 2 and 4 spp, each frame's colour scaled differently, and frame 1's
    channels 9-13 scaled by 8 so that its maxima differ from its neighbours'."""
    if (w, h) not in _base:
        bases, eyes = poses(pt, 4, w, h)
        _base[(w, h)] = [pt.render_frame(w, h, spp, basis=bases[k], eye=eyes[k])[0] for k in range(4) for spp in (2, 4)]
    base = _base[(w, h)]
    out = np.empty((n, h, w, 14), dtype=np.float32)
    for f in range(n):
        out[f] = base[f % len(base)]
        out[f, ..., 0:3] *= np.float32(1.0 + 0.03 * f)
    if n > 1:
        out[1, ..., 9:14] *= np.float32(8.0)
    return out


def sync(pt):
    pt.check(pt.lib.pt_device_synchronize())


def singles(pt, dn, frames, out_of_place):
    """The contract's loop: one pt_denoiser_enqueue per frame of a packed device copy."""
    n, h, w = frames.shape[:3]
    fs = h * w * 14
    d = pt.DeviceBuffer(frames.nbytes).upload(frames)
    d_rgb = pt.DeviceBuffer(n * h * w * 12) if out_of_place else None
    try:
        for f in range(n):
            dn.enqueue(d.ptr + f * fs * 4, d_rgb.ptr + f * h * w * 12 if d_rgb else None)
        sync(pt)
        got = d.download(np.float32, frames.shape)
        return (got, d_rgb.download(np.float32, (n, h, w, 3))) if out_of_place else got
    finally:
        d.free()
        if d_rgb:
            d_rgb.free()


@pytest.fixture(scope="module")
def single_dn(pt, sd):
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = pt.Denoiser(w, h, sd)
        return cache[(w, h)]

    yield get
    for dn in cache.values():
        dn.destroy()


SIZES = [(512, 512), (100, 75), (64, 48), (7, 5), (1, 1)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_batch_equals_single_enqueues(pt, gpu, sd, single_dn, w, h):
    ref_dn = single_dn(w, h)
    for n in (2, 3, 32):
        frames = make_frames(pt, w, h, n)
        dn = pt.Denoiser(w, h, sd, max_frames=n + (n == 3))  # max_frames >= n
        try:
            want = singles(pt, ref_dn, frames, False)
            got = pt.denoise_frames(frames, None, denoiser=dn)
            assert np.array_equal(bits(got), bits(want)), f"{w}x{h} n={n}: in place, all 14 channels"
            want_f, want_rgb = singles(pt, ref_dn, frames, True)
            got_f, got_rgb = pt.denoise_frames(frames, None, out_of_place=True, denoiser=dn)
            assert np.array_equal(bits(got_rgb), bits(want_rgb)), f"{w}x{h} n={n}: out-of-place rgb"
            assert np.array_equal(bits(got_f), bits(frames)), f"{w}x{h} n={n}: frames touched out of place"
            assert np.array_equal(bits(want_f), bits(frames))
        finally:
            dn.destroy()


def test_batch_with_strides_leaves_the_gaps(pt, gpu, sd, single_dn):
    w, h, n = 100, 75, 5
    px = w * h
    fs, rs = px * 14 + 37, px * 3 + 11  # odd gaps: frames are not 16-byte aligned either
    frames = make_frames(pt, w, h, n)
    want = singles(pt, single_dn(w, h), frames, False)
    want_f, want_rgb = singles(pt, single_dn(w, h), frames, True)
    sentinel = np.float32(-1234.5)
    host = np.full(n * fs, sentinel, dtype=np.float32)
    for f in range(n):
        host[f * fs:f * fs + px * 14] = frames[f].ravel()
    dn = pt.Denoiser(w, h, sd, max_frames=n)
    d = pt.DeviceBuffer(host.nbytes).upload(host)
    d_rgb = pt.DeviceBuffer(n * rs * 4).upload(np.full(n * rs, sentinel, dtype=np.float32))
    try:
        dn.denoise_frames(d.ptr, n, fs, d_rgb.ptr, rs)
        got_rgb = d_rgb.download(np.float32, (n * rs,))
        assert np.array_equal(bits(d.download(np.float32, (n * fs,))), bits(host)), "frames touched out of place"
        for f in range(n):
            assert np.array_equal(bits(got_rgb[f * rs:f * rs + px * 3]), bits(want_rgb[f].ravel())), f"rgb of frame {f}"
            assert np.all(got_rgb[f * rs + px * 3:(f + 1) * rs] == sentinel), f"gap after rgb {f}"
        dn.denoise_frames(d.ptr, n, fs)
        got = d.download(np.float32, (n * fs,))
        for f in range(n):
            assert np.array_equal(bits(got[f * fs:f * fs + px * 14]), bits(want[f].ravel())), f"frame {f} in place"
            assert np.all(got[f * fs + px * 14:(f + 1) * fs] == sentinel), f"gap after frame {f}"
    finally:
        d.free()
        d_rgb.free()
        dn.destroy()


def test_groups_and_reserve_no_op(pt, lab, gpu, sd, single_dn):
    w, h, n = 64, 48, 20
    frames = make_frames(pt, w, h, n)
    want = singles(pt, single_dn(w, h), frames, False)
    dn = lab.Denoiser(w, h, sd, max_frames=8)
    try:
        dn.reserve_frames(4)  # smaller: a no-op, groups stay 8, 8, 4
        assert dn.max_frames == 8
        got = lab.denoise_frames(frames, None, denoiser=dn)
        assert np.array_equal(bits(got), bits(want))
        groups, launches = dn.last_enqueue()
        lab.denoise_frame(frames[0], None, denoiser=dn)
        assert groups == 3 and launches == 3 * dn.last_enqueue()[1]
    finally:
        dn.destroy()


def test_a_batch_is_one_group_in_the_launches_of_one_frame(pt, lab, gpu, sd):
    w, h, n = 128, 96, 32
    frames = make_frames(pt, w, h, n)
    dn = lab.Denoiser(w, h, sd, max_frames=n)
    try:
        lab.denoise_frame(frames[0], None, denoiser=dn)
        g1, l1 = dn.last_enqueue()
        assert g1 == 1
        convs = dn.convs()
        assert l1 == 2 + sum(1 + (inf["splits"] > 1) for _, inf in convs)
        lab.denoise_frames(frames, None, denoiser=dn)
        assert dn.last_enqueue() == (1, l1), "32 frames must be ONE group in the launches of one frame"
        layers = dn.layers()
        one, many = dn.conv_plan(1), dn.conv_plan(n)
        for (name, inf), p1, pn in zip(convs, one, many):
            ih, iw, _ = layers[inf["in"]][1]
            oh, ow = (ih - 1) // inf["stride"] + 1, (iw - 1) // inf["stride"] + 1
            assert p1["M"] == oh * ow and (p1["bm"], p1["bn"], p1["splits"]) == (inf["bm"], inf["bn"], inf["splits"]), name
            assert pn["M"] == n * oh * ow, name
            assert (pn["splits"], pn["chunks_per_split"]) == (p1["splits"], p1["chunks_per_split"]), f"{name}: K slicing kept"
    finally:
        dn.destroy()


def test_straight_from_the_renderer(pt, gpu, sd, single_dn):
    """A 32-pose sweep at 512^2 rendered by pt_renderer_enqueue_frames into one strided buffer, denoised by ONE
    enqueue_frames call, equals every frame rendered by Render() and denoised on its own."""
    w, h, n, spp = 512, 512, 32, 2
    px = w * h
    fs = px * 14 + 256
    bases, eyes = poses(pt, n, w, h)
    scene = pt.scene_cornell()
    d_scene, ns = pt.upload_scene(scene)
    r = pt.Renderer(w, h, spp, variant=6)  # (the variant with a frames kernel, whatever the policy would pick)
    assert r.kernel_info(9)["variant"] == 6
    r1 = pt.Renderer(w, h, spp)
    d = pt.DeviceBuffer(n * fs * 4)
    one = pt.DeviceBuffer(px * 56)
    dn = pt.Denoiser(w, h, sd, max_frames=n)
    ref_dn = single_dn(w, h)
    try:
        r.enqueue_frames(d.ptr, fs, d_scene.ptr, ns, bases, eyes)
        assert r.check(wait=True) == 0
        rendered = d.download(np.float32, (n * fs,))
        dn.enqueue_frames(d.ptr, n, fs)
        sync(pt)
        got = d.download(np.float32, (n * fs,))
        for f in range(n):
            r1.render(one.ptr, d_scene.ptr, ns, bases[f], eyes[f])
            frame = one.download(np.float32, (h, w, 14))
            assert np.array_equal(bits(frame.ravel()), bits(rendered[f * fs:f * fs + px * 14])), f"rendered frame {f}"
            ref_dn.denoise(one.ptr)
            want = one.download(np.float32, (px * 14,))
            assert np.array_equal(bits(got[f * fs:f * fs + px * 14]), bits(want)), f"denoised frame {f}"
    finally:
        dn.destroy()
        for b in (d, one, d_scene):
            b.free()
        r.destroy()
        r1.destroy()


def test_runs_are_stable_and_denoisers_independent(pt, gpu, sd):
    fa = make_frames(pt, 100, 75, 3)
    fb = make_frames(pt, 64, 48, 5)
    da = pt.Denoiser(100, 75, sd, max_frames=3)
    db = pt.Denoiser(64, 48, sd, max_frames=5)
    try:
        a0 = pt.denoise_frames(fa, None, out_of_place=True, denoiser=da)[1]
        b0 = pt.denoise_frames(fb, None, denoiser=db)
        for _ in range(2):
            a = pt.denoise_frames(fa, None, out_of_place=True, denoiser=da)[1]
            b = pt.denoise_frames(fb, None, denoiser=db)
            assert np.array_equal(bits(a), bits(a0)) and np.array_equal(bits(b), bits(b0))
    finally:
        da.destroy()
        db.destroy()


def _refused(lab, call, *words):
    with pytest.raises(lab.PtError) as e:
        call()
    assert e.value.code == PT_EINVAL, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_invalid_arguments_launch_nothing(pt, lab, gpu, sd):
    w, h = 7, 5
    px = w * h
    frames = make_frames(pt, w, h, 2)
    dn = lab.Denoiser(w, h, sd, max_frames=2)
    d = lab.DeviceBuffer(frames.nbytes).upload(frames)
    d_rgb = lab.DeviceBuffer(2 * px * 12)
    try:
        lab.denoise_frames(frames, None, denoiser=dn)
        assert dn.last_enqueue()[0] == 1
        calls = [
            (lambda: lab.check(lab.lib.pt_denoiser_enqueue_frames(dn.handle, 2, None, px * 14, None, 0, None)), "d_frames"),
            (lambda: dn.enqueue_frames(d.ptr, 0), "n_frames"),
            (lambda: dn.enqueue_frames(d.ptr, -3), "n_frames"),
            (lambda: dn.enqueue_frames(d.ptr, 2, px * 14 - 1), "frame_stride_floats"),
            (lambda: dn.enqueue_frames(d.ptr, 2, None, d_rgb.ptr, px * 3 - 1), "rgb_stride_floats"),
            (lambda: dn.denoise_frames(d.ptr, 0), "n_frames"),
        ]
        for call, word in calls:
            _refused(lab, call, word)
            assert dn.last_enqueue() == (0, 0), word
        sync(lab)
        assert np.array_equal(bits(d.download(np.float32, frames.shape)), bits(frames)), "a refused call touched the frames"
        _refused(lab, lambda: dn.reserve_frames(0), "max_frames")
        _refused(lab, lambda: dn.reserve_frames(65536), "max_frames")
        thin = lab.Denoiser(4096, 1, sd)
        try:
            _refused(lab, lambda: thin.reserve_frames(16385), "max_frames", "pixels")  # 2^26 pixels + one frame
        finally:
            thin.destroy()
        # the workspace survives the refusals
        assert np.array_equal(bits(lab.denoise_frames(frames, None, denoiser=dn)), bits(singles(lab, dn, frames, False)))
    finally:
        d.free()
        d_rgb.free()
        dn.destroy()
