"""Temporal accumulation with per-pixel motion on the GPU (pt_temporal_motion, the _motion and _scene calls; csrc/pt_temporal.hip)
against the float32 model (tests/temporal_motion_model.py), every comparison bit for bit: the motion kernel on Cornell's spheres
at 33 x 20, on open random scenes that cross the staging chunk once and twice, with the winner on either side of a chunk border
and with duplicated spheres; the accumulate kernel with hand-made motion images (uniform, on half the frame, out of the frame,
NaN and infinite) on integer-built frames at 19 x 13 and 64 x 32; a zero motion image against no motion image; a rendered
sequence with a moving sphere through the _scene calls, frame by frame and as one batch, with a reset in the middle and the
workspace figure; the refusals on a live session; and `pathtrace --velocities --temporal`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import temporal_exact_cases as tx
import temporal_model as tm
import temporal_motion_model as mm
import temporal_motion_refusal_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 4
CHUNK = mm.MOTION_CHUNK
EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    """Equal bits, or NaN on both sides (a NaN that passes through keeps no promised payload)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    bad = np.argwhere(~same_bits(got, want))
    assert bad.size == 0, (what, len(bad), bad[:5], [(got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


# ---- the motion image -----------------------------------------------------------------------------------------------------

def gpu_motion(pt, w, h, now, prev, basis, eye):
    """pt_temporal_motion into a device buffer of the test's own, on a fresh session."""
    ta = pt.Temporal(w, h)
    d = pt.DeviceBuffer(w * h * 16)
    try:
        d.upload(np.full((h, w, 4), -7.0, f32))
        _, b = pt._f32(basis, 12)
        _, e = pt._f32(eye, 3)
        now, prev = np.ascontiguousarray(now), np.ascontiguousarray(prev)
        pt.check(pt.lib.pt_temporal_motion(ta.handle, now.ctypes.data, prev.ctypes.data, len(now), b, e, d.ptr, None))
        pt.check(pt.lib.pt_device_synchronize())
        assert ta.memory()["workspace"] == w * h * 96  # (the session's own motion image is not needed for this call)
        return d.download(f32, (h, w, 4))
    finally:
        d.free()
        ta.destroy()


def moved(spheres, seed):
    """The scene one frame earlier: every centre displaced by a few units."""
    prev = spheres.copy()
    prev["pos"] -= np.random.default_rng(seed).integers(-8, 9, prev["pos"].shape).astype(f32) / f32(4.0)
    return prev


def test_motion_image_of_the_cornell_box_at_33x20(pt, gpu):
    w, h = 33, 20
    now, basis = pt.scene_cornell(), pt.camera_basis(width=w, height=h)
    prev = now.copy()
    prev["pos"][7] -= np.array([2.5, 0.0, 1.0], f32)
    prev["pos"][8] -= np.array([0.0, 0.125, -3.0], f32)
    prev["pos"][1] -= np.array([0.5, 0.0, 0.0], f32)
    want = mm.motion_image(w, h, now, prev, basis, pt.DEFAULT_EYE)
    # (the frame is not square, so the view is stretched: walls 0, 1, 2, 5 and the right sphere; a closed box: every ray hits)
    assert {1.0, 8.0} <= set(np.unique(want[..., 3])) and len(np.unique(want[..., 3])) >= 5 and (want[..., 3] >= 0).all()
    assert_same(gpu_motion(pt, w, h, now, prev, basis, pt.DEFAULT_EYE), want, "cornell")


@pytest.mark.parametrize("n", [CHUNK + 1, 2 * CHUNK + 3], ids=["chunk+1", "2chunk+3"])
def test_motion_image_of_open_random_scenes_across_the_staging_chunk(pt, gpu, n):
    w = h = 16
    now, basis = pt.scene_random(n, 5, False), pt.camera_basis(width=w, height=h)
    prev = moved(now, n)
    want = mm.motion_image(w, h, now, prev, basis, pt.DEFAULT_EYE)
    index = want[..., 3]
    assert (index < 0).any() and (index >= 0).any()  # (the open scene: misses occur)
    if n > 2 * CHUNK:
        assert (index >= CHUNK).any() and ((index >= 0) & (index < CHUNK)).any()  # (winners from more than one round)
    assert_same(gpu_motion(pt, w, h, now, prev, basis, pt.DEFAULT_EYE), want, n)


def crafted_scene(pt, n, near, far):
    """n spheres behind the eye of tx's camera, which no ray hits, but two in front of it: `near` (radius 30 at distance 40,
    which covers 48.6 degrees around the axis) and `far` (radius 80 at distance 100: 53.1 degrees, visible around `near`; the corner
    rays, 57 degrees off the axis, miss both)."""
    eye = tx.EYE.astype(f32)
    s = np.zeros(n, pt.SPHERE_DTYPE)
    s["radius"], s["color"] = 1.0, 0.5
    s["pos"] = eye + np.stack([np.zeros(n), np.zeros(n), 500.0 + np.arange(n)], axis=1).astype(f32)
    for where, distance, radius in zip((near, far), (40.0, 100.0), (30.0, 80.0)):
        for i in np.atleast_1d(where):
            s["pos"][i], s["radius"][i] = eye + np.array([0.0, 0.0, -distance], f32), radius
    return s


@pytest.mark.parametrize("near,far,winner", [
    (CHUNK - 1, 0, CHUNK - 1), (CHUNK - 1, CHUNK, CHUNK - 1),  # the winner is the last sphere of a round
    (CHUNK, CHUNK - 1, CHUNK), (CHUNK, 2 * CHUNK + 1, CHUNK),  # the winner is the first sphere of the next round
    ([3, CHUNK + 1], 1, 3), ([CHUNK - 1, CHUNK], [2 * CHUNK - 1, 2 * CHUNK], CHUNK - 1),  # identical spheres: the lower index
], ids=["last-of-round", "last-of-round-far-behind", "first-of-next", "first-of-next-far-behind", "twins", "twins-across-rounds"])
def test_motion_image_picks_the_winner_on_either_side_of_a_round(pt, gpu, near, far, winner):
    w = h = 16
    now = crafted_scene(pt, 2 * CHUNK + 2, near, far)
    prev = moved(now, 9)
    want = mm.motion_image(w, h, now, prev, tx.BASIS, tx.EYE)
    index = want[..., 3]
    assert index[12, 4] == winner and (index == np.atleast_1d(far).min()).any() and (index < 0).any()
    assert set(np.unique(index)) == {-1.0, float(winner), float(np.atleast_1d(far).min())}
    assert_same(gpu_motion(pt, w, h, now, prev, tx.BASIS, tx.EYE), want, (near, far))


def test_motion_through_the_wrapper_into_a_buffer_and_on_to_run(pt, gpu):
    """Temporal.motion(out=) and run(motion=) with the same DeviceBuffer: the model's motion image and the model's frame."""
    w, h = 33, 20
    now, basis = pt.scene_cornell(), pt.camera_basis(width=w, height=h)
    prev = moved(now, 3)
    frames = [tx.make_frame(w, h, 401), tx.make_frame(w, h, 402)]
    for F in frames:
        F[..., 9] = 8192.0  # (the Camera's directions are short: this is some 200 units away, where the box is)
    model = mm.MotionTemporalModel(w, h)
    want_motion = mm.motion_image(w, h, now, prev, basis, pt.DEFAULT_EYE)
    model.accumulate(frames[0], N, basis, pt.DEFAULT_EYE)
    want = model.accumulate(frames[1], N, basis, pt.DEFAULT_EYE, motion=want_motion)
    static = tm.run_calls(w, h, [(F, N, basis, pt.DEFAULT_EYE) for F in frames])[0][1]
    assert (want[1] > N).mean() > 0.5 and not same_bits(want[0], static).all()  # (history is found, and not where it was)
    ta = pt.Temporal(w, h)
    d_frame, d_counts, d_motion = pt.DeviceBuffer(h * w * 14 * 4), pt.DeviceBuffer(h * w * 4), pt.DeviceBuffer(h * w * 16)
    try:
        ta.run(d_frame.upload(frames[0]).ptr, N, basis)
        assert ta.motion(now, prev, basis, out=d_motion) is d_motion
        ta.run(d_frame.upload(frames[1]).ptr, N, basis, d_counts=d_counts.ptr, motion=d_motion)
        assert_same(d_motion.download(f32, (h, w, 4)), want_motion, "Temporal.motion")
        assert_same(d_frame.download(f32, (h, w, 14)), want[0], "run(motion=)")
        assert np.array_equal(d_counts.download(np.uint32, (h, w)), want[1])
    finally:
        for d in (d_frame, d_counts, d_motion):
            d.free()
        ta.destroy()


# ---- accumulation with a motion image ---------------------------------------------------------------------------------------

U = np.array([3.0, -2.0, 1.5], f32)


def motion_images(W, H):
    """name -> (motion [H][W][4], eye of the second call, pixels that must restart or None, least share kept or None)."""
    def image(m):
        out = np.zeros((H, W, 4), f32)
        out[..., :3] = m
        return out
    uniform = image(U)
    half = image(U)
    half[:, W // 2:, :3] = 0.0
    half[:, W // 2:, 3] = -1.0
    outside = image((4096.0, 0.0, 0.0))
    broken = image(0.0)
    spots = [(1, 2, 0, np.nan), (3, 5, 1, np.inf), (5, 7, 2, -np.inf), (H - 1, W - 1, 0, np.nan), (0, 0, 1, np.inf)]
    for r, c, k, v in spots:
        broken[r, c, k] = v
    restart = np.zeros((H, W), bool)
    for r, c, _, _ in spots:
        restart[r, c] = True
    return {
        "uniform": (uniform, tx.EYE + U, None, 0.9),       # the eye moves with the world: every pixel finds itself
        "uniform-still-eye": (uniform, tx.EYE, None, None),  # the world moves under a camera at rest
        "half": (half, tx.EYE, None, 0.45),                 # the right half is static
        "outside": (outside, tx.EYE, np.ones((H, W), bool), None),
        "nonfinite": (broken, tx.EYE, restart, 0.9),
    }


def run_motion_calls(pt, W, H, calls):
    """calls [(frame, basis, eye, motion or None)] through Temporal.run on one session: ([frames], [counts])."""
    ta = pt.Temporal(W, H, **tx.OPTS)
    d_frame, d_counts, d_motion = pt.DeviceBuffer(H * W * 14 * 4), pt.DeviceBuffer(H * W * 4), pt.DeviceBuffer(H * W * 16)
    outs, counts = [], []
    try:
        for F, b, e, m in calls:
            d_frame.upload(F)
            if m is not None:
                d_motion.upload(m)
            assert ta.run(d_frame.ptr, N, b, e, d_counts=d_counts.ptr, motion=d_motion if m is not None else None) >= 0
            outs.append(d_frame.download(f32, (H, W, 14)))
            counts.append(d_counts.download(np.uint32, (H, W)))
        assert ta.memory()["workspace"] == W * H * 96  # (a caller's motion image costs the session nothing)
    finally:
        for d in (d_frame, d_counts, d_motion):
            d.free()
        ta.destroy()
    return outs, counts


@pytest.mark.parametrize("name", ["uniform", "uniform-still-eye", "half", "outside", "nonfinite"])
@pytest.mark.parametrize("size", [(19, 13), (64, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulation_with_a_motion_image_equals_the_model(pt, gpu, size, name):
    """Three calls: plain, with the motion image, plain again (the state the motion call left)."""
    W, H = size
    motion, eye2, restart, share = motion_images(W, H)[name]
    frames = [tx.make_frame(W, H, 201 + i) for i in range(3)]
    calls = [(frames[0], tx.BASIS, tx.EYE, None), (frames[1], tx.BASIS, eye2, motion), (frames[2], tx.BASIS, eye2, None)]
    model = mm.MotionTemporalModel(W, H, **tx.OPTS)
    want = [model.accumulate(F, N, b, e, motion=m) for F, b, e, m in calls]
    kept = want[1][1] > N
    if restart is not None:  # the model restarts exactly there, as it does for a NaN depth
        assert not kept[restart].any() and same_bits(want[1][0][restart], frames[1][restart]).all()
    if share is not None:
        assert kept.mean() >= share, kept.mean()
    if name == "half":
        assert kept[:, W // 2 + 1:].all()
    outs, counts = run_motion_calls(pt, W, H, calls)
    for i in range(3):
        assert_same(outs[i], want[i][0], (name, i))
        assert np.array_equal(counts[i], want[i][1]), (name, i)


def test_a_zero_motion_image_is_no_motion_image(pt, gpu):
    """The frame, the counts and the next call's output, bit for bit -- through run and through enqueue."""
    W, H = 64, 32
    frames = [tx.make_frame(W, H, 301 + i) for i in range(3)]
    eyes = [tx.shifted_eye(W, H, 1.5, -0.5), tx.shifted_eye(W, H, 0.5, 0), tx.EYE]
    zero = np.zeros((H, W, 4), f32)
    zero[::2, :, 3] = -1.0
    plain = run_motion_calls(pt, W, H, [(F, tx.BASIS, e, None) for F, e in zip(frames, eyes)])
    with_zero = run_motion_calls(pt, W, H, [(F, tx.BASIS, e, zero if i == 1 else None) for i, (F, e) in enumerate(zip(frames, eyes))])
    assert (plain[1][1] > N).mean() > 0.9 and (plain[1][2] > 2 * N).mean() > 0.9
    for i in range(3):
        assert np.array_equal(bits(plain[0][i]), bits(with_zero[0][i])) and np.array_equal(plain[1][i], with_zero[1][i]), i
    # enqueue(motion=) on the default stream
    ta = pt.Temporal(W, H, **tx.OPTS)
    bufs = [pt.DeviceBuffer(H * W * 14 * 4).upload(F) for F in frames]
    d_counts, d_zero = pt.DeviceBuffer(H * W * 4), pt.DeviceBuffer(H * W * 16).upload(zero)
    try:
        for i, (d, e) in enumerate(zip(bufs, eyes)):
            ta.enqueue(d.ptr, N, tx.BASIS, e, d_counts=d_counts.ptr, motion=d_zero.ptr if i == 1 else None)
        pt.check(pt.lib.pt_device_synchronize())
        for i, d in enumerate(bufs):
            assert np.array_equal(bits(d.download(f32, (H, W, 14))), bits(plain[0][i])), i
        assert np.array_equal(d_counts.download(np.uint32, (H, W)), plain[1][2])
        with pytest.raises(ValueError):
            ta.enqueue(bufs[0].ptr, N, tx.BASIS, tx.EYE, motion=d_zero.ptr, spheres=pt.scene_cornell())
    finally:
        for d in bufs + [d_counts, d_zero]:
            d.free()
        ta.destroy()


# ---- _scene sessions ----------------------------------------------------------------------------------------------------------

SIZE, FRAMES, MOVING, VELOCITY = 64, 6, 7, (2.5, 0.0, 1.0)
_cache = {}


def rendered(pt, rng="philox", frames=FRAMES):
    """The frames of the 64 x 64 Cornell box with sphere 7 in motion from the project's own Renderer (4 spp, one renderer for the
    sequence), their scenes [K][9], cameras, and the model's frames and counts; rendered once, read-only."""
    if (rng, frames) not in _cache:
        cornell = pt.scene_cornell()
        scenes = np.stack([mm.moved_scene(cornell, {MOVING: VELOCITY}, k) for k in range(frames)])
        basis = pt.camera_basis(width=SIZE, height=SIZE)
        bases, eyes = np.stack([basis] * frames), np.asarray([pt.DEFAULT_EYE] * frames, f32)
        r = pt.Renderer(SIZE, SIZE, N, rng_mode=pt.RNG_PHILOX if rng == "philox" else pt.RNG_XORWOW)
        d_scene, ns = pt.upload_scene(cornell)
        d_out = pt.DeviceBuffer(SIZE * SIZE * 14 * 4)
        try:
            out = []
            for k in range(frames):
                d_scene.upload(scenes[k])
                r.render(d_out.ptr, d_scene.ptr, ns, basis, pt.DEFAULT_EYE)
                out.append(d_out.download(f32, (SIZE, SIZE, 14)))
        finally:
            d_out.free()
            d_scene.free()
            r.destroy()
        out = np.stack(out)
        want, want_counts = mm.accumulate_scenes(out, N, bases, eyes, scenes)
        for a in (out, scenes, bases, eyes, want, want_counts):
            a.setflags(write=False)
        _cache[(rng, frames)] = (out, scenes, bases, eyes, want, want_counts)
    return _cache[(rng, frames)]


def test_scene_sessions_follow_a_moving_sphere(pt, gpu):
    """Frame by frame through enqueue(spheres=) and run(spheres=), and all at once through enqueue_frames(scenes=): the model's
    bits, and the same bits both ways.  The workspace grows by 16 bytes per pixel exactly once, at the second call."""
    frames, scenes, bases, eyes, want, want_counts = rendered(pt)
    px = SIZE * SIZE
    on_sphere = mm.motion_image(SIZE, SIZE, scenes[-1], scenes[-2], bases[-1], eyes[-1])[..., 3] == MOVING
    assert on_sphere.sum() > 50 and (want_counts[-1][on_sphere] > N).mean() > 0.5  # (the moving sphere keeps its history)
    blind, _ = tm.accumulate_sequence(frames, N, bases, eyes)
    assert not np.array_equal(bits(blind[-1]), bits(want[-1]))  # (and the motion matters)
    ta = pt.Temporal(SIZE, SIZE)
    d_frame, d_counts = pt.DeviceBuffer(px * 14 * 4), pt.DeviceBuffer(px * 4)
    try:
        memory = []
        for k in range(FRAMES):
            d_frame.upload(frames[k])
            if k % 2:
                assert ta.run(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scenes[k]) >= 0
            else:
                ta.enqueue(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scenes[k])
                pt.check(pt.lib.pt_device_synchronize())
            memory.append(ta.memory()["workspace"])
            assert_same(d_frame.download(f32, (SIZE, SIZE, 14)), want[k], ("single", k))
            assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), want_counts[k]), k
        assert memory == [px * 96] + [px * 112] * (FRAMES - 1)
    finally:
        d_frame.free()
        d_counts.free()
        ta.destroy()
    singles = want  # (asserted equal to every single call's frame above)
    # all six in ONE enqueue_frames(scenes=) call (pt_temporal_enqueue_frames_scenes), 37 floats of sentinel behind every frame
    stride, sentinel = px * 14 + 37, f32(-12345.5)
    host = np.full((FRAMES, stride), sentinel, f32)
    host[:, :px * 14] = frames.reshape(FRAMES, -1)
    ta = pt.Temporal(SIZE, SIZE)
    d_frames, d_counts = pt.DeviceBuffer(host.nbytes).upload(host), pt.DeviceBuffer(px * 4)
    try:
        ta.enqueue_frames(d_frames.ptr, N, bases, eyes, frame_stride_floats=stride, d_counts=d_counts.ptr, scenes=scenes)
        pt.check(pt.lib.pt_device_synchronize())
        got = d_frames.download(f32, (FRAMES, stride))
        assert (got[:, px * 14:] == sentinel).all()
        got = np.ascontiguousarray(got[:, :px * 14]).reshape(frames.shape)
        assert_same(got, want, "enqueue_frames(scenes=)")
        assert np.array_equal(bits(got), bits(singles))
        assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), want_counts[-1])
        assert ta.memory()["workspace"] == px * 112
        # and the session it leaves goes on as the single calls' would: frame 4 again, following the sphere back from frame 5
        d_frames.upload(frames[4])
        ta.enqueue(d_frames.ptr, N, bases[4], eyes[4], d_counts=d_counts.ptr, spheres=scenes[4])
        model = mm.MotionTemporalModel(SIZE, SIZE)
        for k in range(FRAMES):
            model.accumulate_scene(frames[k], N, bases[k], eyes[k], scenes[k])
        again = model.accumulate_scene(frames[4], N, bases[4], eyes[4], scenes[4])
        assert_same(d_frames.download(f32, (FRAMES, stride))[0, :px * 14].reshape(SIZE, SIZE, 14), again[0], "after the batch")
        assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), again[1])
    finally:
        d_frames.free()
        d_counts.free()
        ta.destroy()
    # the synchronous twin through the convenience (pt_temporal_run_frames_scenes)
    got, last_counts = pt.accumulate_frames(frames, N, bases, eyes, scenes=scenes)
    assert_same(got, want, "run_frames(scenes=)")
    assert np.array_equal(last_counts, want_counts[-1])


def test_scene_session_reset_plain_calls_and_refusals(pt, gpu):
    """On one session: a reset in the middle passes the next frame through and forgets the scene (another sphere count is then
    welcome); a plain call forgets the scene, so the next _scene call accumulates with zero motion; a refused call -- every case
    of temporal_motion_refusal_cases that concerns a scene, another n, another radius -- leaves history, scene and workspace as
    they were."""
    frames, scenes, bases, eyes, _, _ = rendered(pt)
    px = SIZE * SIZE
    model = mm.MotionTemporalModel(SIZE, SIZE)
    ta = pt.Temporal(SIZE, SIZE)
    d_frame, d_counts = pt.DeviceBuffer(px * 14 * 4), pt.DeviceBuffer(px * 4)
    extra = np.concatenate([scenes[2], scenes[2][7:8]])  # ten spheres

    def both(k, how, scene=None):
        d_frame.upload(frames[k])
        if how == "scene":
            ta.run(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr, spheres=scene)
            want = model.accumulate_scene(frames[k], N, bases[k], eyes[k], scene)
        else:
            ta.run(d_frame.ptr, N, bases[k], eyes[k], d_counts=d_counts.ptr)
            want = model.accumulate(frames[k], N, bases[k], eyes[k])
        assert_same(d_frame.download(f32, (SIZE, SIZE, 14)), want[0], (k, how))
        assert np.array_equal(d_counts.download(np.uint32, (SIZE, SIZE)), want[1]), (k, how)
        return want

    def refused(k, scene, word, basis=None, n=None):
        """run(spheres=scene); with n: pt_temporal_run_scene itself with that count (scene None: a null h_spheres)."""
        d_frame.upload(frames[k])
        before = ta.memory()["workspace"]
        with pytest.raises(pt.PtError) as err:
            if n is None:
                ta.run(d_frame.ptr, N, bases[k] if basis is None else basis, eyes[k], d_counts=d_counts.ptr, spheres=scene)
            else:
                _, b = pt._f32(bases[k], 12)
                _, e = pt._f32(eyes[k], 3)
                pt.check(pt.lib.pt_temporal_run_scene(ta.handle, d_frame.ptr, N, b, e, rc.pointer(scene), n, d_counts.ptr, None))
        assert err.value.code == rc.PT_EINVAL and word in str(err.value) and "pt_temporal_run_scene" in str(err.value), str(err.value)
        assert np.array_equal(bits(d_frame.download(f32, (SIZE, SIZE, 14))), bits(frames[k]))  # nothing was launched
        assert ta.memory()["workspace"] == before

    try:
        both(0, "scene", scenes[0])
        both(1, "scene", scenes[1])
        refused(2, extra, "n 10 differs from the 9 spheres")
        changed = scenes[2].copy()
        changed["radius"][MOVING] = 16.0
        refused(2, changed, "reset the session")
        refused(2, None, "null h_spheres", n=9)
        big = np.zeros(65536, pt.SPHERE_DTYPE)
        for n, word in ((0, "n 0 outside 1 .. 65535"), (-4, "n -4 outside"), (65536, "n 65536 outside")):
            refused(2, big, word, n=n)
        for name, edit, word in rc.CASES:
            if name.startswith("basis-"):
                refused(2, scenes[2], word, basis=rc.arguments(pt, edit)["basis"])
        for name, edit, word in rc.CASES:
            a = rc.arguments(pt, edit)
            if a["now"] is not None and a["n"] == 9 and name.endswith(("-now", "radius", "color")) and "changed" not in name:
                refused(2, a["now"], word.replace("h_now", "h_spheres"))
        assert (both(2, "scene", scenes[2])[1] > 2 * N).any()  # the session is as it was: frame 2 follows frame 1
        ta.reset()
        model.reset()
        out = both(3, "scene", extra)  # passes through, remembers ten spheres
        assert (out[1] == N).all() and np.array_equal(bits(out[0]), bits(frames[3]))
        refused(4, scenes[4], "n 9 differs from the 10 spheres")
        both(4, "plain")  # forgets the scene
        out = both(5, "scene", scenes[5])  # nine spheres again: zero motion, and frame 5 accumulates over frames 3 and 4
        assert (out[1] == 3 * N).mean() > 0.5
        both(5, "scene", scenes[4])  # and that call remembered its scene: this one follows the sphere (backwards)
    finally:
        d_frame.free()
        d_counts.free()
        ta.destroy()


def test_motion_refusals_on_a_live_session_launch_nothing(pt, gpu):
    """Every case of temporal_motion_refusal_cases through pt_temporal_motion: PT_EINVAL naming the argument, the output buffer
    untouched, and the session works afterwards."""
    w = h = 64
    ta = pt.Temporal(w, h)
    d = pt.DeviceBuffer(w * h * 16)
    sentinel = np.full((h, w, 4), -7.0, f32)
    fp = ctypes.c_float
    try:
        d.upload(sentinel)
        for name, edit, word in rc.CASES:
            a = rc.arguments(pt, edit)
            code = pt.lib.pt_temporal_motion(ta.handle, rc.pointer(a["now"]), rc.pointer(a["prev"]), a["n"], rc.pointer(a["basis"], fp),
                                             rc.pointer(a["eye"], fp), d.ptr, None)
            msg = pt.lib.pt_last_error().decode()
            assert code == rc.PT_EINVAL and word in msg and "pt_temporal_motion" in msg, (name, code, msg)
        a = rc.arguments(pt, lambda *x: None)
        assert pt.lib.pt_temporal_motion(ta.handle, rc.pointer(a["now"]), rc.pointer(a["prev"]), 9, rc.pointer(a["basis"], fp),
                                         rc.pointer(a["eye"], fp), None, None) == rc.PT_EINVAL
        assert "null d_motion" in pt.lib.pt_last_error().decode()
        pt.check(pt.lib.pt_device_synchronize())
        assert np.array_equal(d.download(f32, (h, w, 4)), sentinel)
        ta.motion(a["now"], a["prev"], a["basis"], a["eye"], out=d)
        pt.check(pt.lib.pt_device_synchronize())
        assert_same(d.download(f32, (h, w, 4)), mm.motion_image(w, h, a["now"], a["prev"], a["basis"], a["eye"]), "after the refusals")
    finally:
        d.free()
        ta.destroy()


# ---- the CLI --------------------------------------------------------------------------------------------------------

def _read_exr(path, w, h):
    raw = open(path, "rb").read()
    block = 8 + w * 14 * 4
    data = raw[len(raw) - h * block:]
    out = np.empty((h, w, 14), f32)
    for y in range(h):
        row = np.frombuffer(data, dtype="<f4", count=w * 14, offset=y * block + 8).reshape(14, w)
        for c in range(14):
            out[y, :, EXR_SOURCE[c]] = row[c]
    return out


def test_cli_velocities_with_temporal_writes_the_predicted_frame(pt, gpu, tmp_path):
    """pathtrace --size 64 -s 4 --frames 4 --velocities F [--temporal]: without --temporal the saved EXR is the plain render of
    the last frame's scene, with it the model's last frame, the model fed with what a default Renderer produces."""
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    frames, scenes, bases, eyes, want, _ = rendered(pt, "xorwow", 4)
    (tmp_path / "v.txt").write_text("# the left sphere\n%d %r %r %r\n" % ((MOVING,) + VELOCITY))
    outs = {}
    for name, extra in (("plain", []), ("temporal", ["--temporal"])):
        o = str(tmp_path / name)
        run = subprocess.run([exe, "--size", "64", "-s", str(N), "--frames", "4", "--velocities", "v.txt", "--nobitmap", "-o", o] + extra,
                             capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert run.returncode == 0, run.stderr
        outs[name] = _read_exr(o + ".exr", 64, 64)
    assert np.array_equal(bits(outs["plain"]), bits(frames[-1]))  # the test renders what the command renders
    assert not np.array_equal(bits(want[-1]), bits(frames[-1]))
    assert np.array_equal(bits(outs["temporal"]), bits(want[-1]))
