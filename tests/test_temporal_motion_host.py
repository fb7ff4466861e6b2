"""CPU tests of temporal accumulation with per-pixel motion (pt_temporal_motion and the _motion / _scene calls; DENOISER.md,
"Moving spheres"): the float32 model (tests/temporal_motion_model.py) against TemporalModel for a zero motion image, against
closed forms for the motion image and against a still world for a world that moves rigidly with the camera; the model's quality on
oracle frames of a Cornell box with one sphere in motion; the host refusals of the C ABI; the parse errors of
`pathtrace --velocities`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import temporal_exact_cases as tx
import temporal_model as tm
import temporal_motion_model as mm
import temporal_motion_refusal_cases as rc
from conftest import ROOT

f32, f64 = np.float32, np.float64
SYMBOLS = ("pt_temporal_scene_check", "pt_temporal_motion", "pt_temporal_enqueue_motion", "pt_temporal_run_motion",
           "pt_temporal_enqueue_scene", "pt_temporal_run_scene", "pt_temporal_enqueue_frames_scenes", "pt_temporal_run_frames_scenes")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def sphere(pt, pos, radius):
    s = np.zeros(1, pt.SPHERE_DTYPE)
    s["pos"], s["radius"], s["color"] = pos, radius, 0.5
    return s


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert f"#define PT_MOTION_CHUNK {pt.MOTION_CHUNK}\n" in header and pt.MOTION_CHUNK == mm.MOTION_CHUNK


@pytest.mark.parametrize("name,edit,word", rc.CASES, ids=rc.IDS)
def test_scene_check_refuses_before_a_device_is_touched(pt, name, edit, word):
    """PT_EINVAL naming the argument, on a machine without a GPU too; the model refuses the same scenes."""
    a = rc.arguments(pt, edit)
    fp = ctypes.c_float
    code = pt.lib.pt_temporal_scene_check(rc.pointer(a["now"]), rc.pointer(a["prev"]), a["n"], rc.pointer(a["basis"], fp), rc.pointer(a["eye"], fp))
    msg = pt.lib.pt_last_error().decode()
    assert code == rc.PT_EINVAL and word in msg and "pt_temporal_scene_check" in msg, (code, msg)
    if all(a[k] is not None for k in ("now", "prev", "basis", "eye")) and a["n"] == 9 and np.isfinite(a["eye"]).all():
        with pytest.raises(ValueError):
            mm.motion_image(64, 64, a["now"], a["prev"], a["basis"], a["eye"])


def test_scene_check_accepts_what_differs_only_in_position_colour_and_emission(pt):
    a = rc.arguments(pt, lambda *x: None)
    a["prev"]["color"][7], a["prev"]["emission"][2] = (0.1, 0.2, 0.3), (5.0, 0.0, 1.0)
    pt.temporal_scene_check(a["now"], a["prev"], a["basis"], a["eye"])
    pt.temporal_scene_check(pt.scene_random(65535, 1, False), pt.scene_random(65535, 1, False), a["basis"], a["eye"])


def test_null_sessions_are_refused_without_a_device(pt):
    L = pt.lib
    for call, word in [
        (lambda: L.pt_temporal_motion(None, None, None, 9, None, None, None, None), "null accumulator"),
        (lambda: L.pt_temporal_enqueue_motion(None, None, 4, None, None, None, None, None), "null accumulator"),
        (lambda: L.pt_temporal_run_motion(None, None, 4, None, None, None, None, None), "null accumulator"),
        (lambda: L.pt_temporal_enqueue_scene(None, None, 4, None, None, None, 9, None, None), "null accumulator"),
        (lambda: L.pt_temporal_run_scene(None, None, 4, None, None, None, 9, None, None), "null accumulator"),
        (lambda: L.pt_temporal_enqueue_frames_scenes(None, 2, None, 14, None, None, None, 9, 4, None, None), "null accumulator"),
        (lambda: L.pt_temporal_run_frames_scenes(None, 2, None, 14, None, None, None, 9, 4, None, None), "null accumulator"),
    ]:
        assert call() == rc.PT_EINVAL
        assert word in L.pt_last_error().decode()


# ---- a zero motion image ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tx.CASES + tx.NONFINITE, ids=repr)
def test_zero_motion_equals_the_static_model_bit_for_bit(case):
    """x - 0.0f is x for every float, NaN and -0 included."""
    want, want_counts = tm.run_calls(case.W, case.H, case.calls, **case.opts)
    m = mm.MotionTemporalModel(case.W, case.H, **case.opts)
    zero = np.zeros((case.H, case.W, 4), f32)
    zero[..., 3] = -1.0
    for i, (F, n, b, e) in enumerate(case.calls):
        out, counts = m.accumulate(F, n, b, e, motion=zero)
        assert same_bits(out, want[i]) and np.array_equal(counts, want_counts[i]), (case.name, i)


# ---- the motion image in closed form ----------------------------------------------------------------------------------------

W16 = 16  # with tx.BASIS at 16 x 16: d = (-0.5 + c / 8, 0.75 - r / 16, -1)


def test_motion_image_closed_forms(pt):
    """Pixel (row 12, column 4) looks along d = (0, 0, -1): a sphere of radius 2 centred at eye + 8 d has b = -16, c = 60,
    det = 16, roots 6 and 10.  Pixel (row 12, column 10) looks along d = (0.75, 0, -1), |d|^2 = 1.5625: radius 2.5 at eye + 8 d
    has b = -25, c = 93.75, det = 39.0625, roots 6 and 10.  Every number is dyadic, so float32 and the reference's mixed
    arithmetic give them exactly."""
    eye = tx.EYE.astype(f32)
    o, d = mm.nr._primary(W16, W16, tx.BASIS, eye)
    assert [float(d[k][12, 4]) for k in range(3)] == [0.0, 0.0, -1.0] and [float(d[k][12, 10]) for k in range(3)] == [0.75, 0.0, -1.0]
    a = sphere(pt, eye + 8 * np.array([0.0, 0.0, -1.0], f32), 2.0)
    b = sphere(pt, eye + 8 * np.array([0.75, 0.0, -1.0], f32), 2.5)
    behind = sphere(pt, eye - 8 * np.array([0.0, 0.0, -1.0], f32), 2.0)  # the same sphere behind the eye: both roots negative
    now = np.concatenate([behind, a, b, a])  # (index 3 repeats index 1)
    prev = now.copy()
    prev["pos"] -= np.array([1.0, 0.5, -2.0], f32)
    prev["pos"][2] = now["pos"][2] - np.array([0.25, 0.0, 4.0], f32)
    hit, t, index = mm.first_hit(W16, W16, now, tx.BASIS, eye)
    assert hit[12, 4] and t[12, 4] == 6.0 and index[12, 4] == 1  # strict <: the duplicate at index 3 never wins
    assert hit[12, 10] and t[12, 10] == 6.0 and index[12, 10] == 2
    assert not (index == 3).any() and not (index[hit] == 0).any()
    m = mm.motion_image(W16, W16, now, prev, tx.BASIS, eye)
    assert m[12, 4].tolist() == [1.0, 0.5, -2.0, 1.0] and m[12, 10].tolist() == [0.25, 0.0, 4.0, 2.0]
    assert not hit[0, 0] and m[0, 0].tolist() == [0.0, 0.0, 0.0, -1.0]
    # the sphere behind the eye alone: every pixel misses
    m = mm.motion_image(W16, W16, behind, behind, tx.BASIS, eye)
    assert (m[..., 3] == -1.0).all() and (m[..., :3] == 0.0).all()


# ---- a world that moves rigidly with the camera -------------------------------------------------------------------------------

U = np.array([3.0, -2.0, 1.5])  # the world's step between the two frames


def rigid_pair(pt, W, H, k, j):
    """(still, moved): two-call sequences as (frame, n, basis, eye, scene).  still: the camera shifts by (k, j) pixels in front
    of a scene at rest.  moved: the same, and between the calls the eye and every sphere also move by U.  One sphere of radius
    1024 around the eye covers every pixel."""
    F1, F2 = tx.make_frame(W, H, 101), tx.make_frame(W, H, 102)
    eye1, eye2 = tx.shifted_eye(W, H, k, j), tx.EYE
    scene = np.concatenate([sphere(pt, (48.0, 48.0, 256.0), 1024.0), sphere(pt, (48.0, 48.0, 4096.0), 8.0)])
    scene2 = scene.copy()
    scene2["pos"] = scene["pos"] + U.astype(f32)
    still = [(F1, tx.N, tx.BASIS, eye1, scene), (F2, tx.N, tx.BASIS, eye2, scene)]
    moved = [(F1, tx.N, tx.BASIS, eye1, scene), (F2, tx.N, tx.BASIS, eye2 + U, scene2)]
    return still, moved


def assert_rigid_premise(W, H, still, moved):
    """Every intermediate of the extra steps is exact in float32: X = eye + d z, Xp = X - U and q = Xp - eye' of the moved
    sequence, and q equals the still sequence's."""
    r, c = (a.astype(f64) for a in np.mgrid[0:H, 0:W])
    d = tx.B0 + (c / H)[..., None] * tx.E1 + (1.0 - r / W)[..., None] * tx.E2
    z = moved[1][0][..., 9].astype(f64)[..., None]
    X_still, X_moved = np.asarray(still[1][3], f64) + d * z, np.asarray(moved[1][3], f64) + d * z
    Xp = X_moved - U
    q_still, q_moved = X_still - np.asarray(still[0][3], f64), Xp - np.asarray(moved[0][3], f64)
    for a in (d, d * z, X_still, X_moved, Xp, q_still, q_moved, moved[1][3], moved[1][4]["pos"].astype(f64)):
        assert tx.is_f32(a)
    assert np.array_equal(q_still, q_moved) and np.array_equal(Xp, X_still)


@pytest.mark.parametrize("W,H,k,j", [(64, 32, 0, 0), (64, 32, 3, 0), (32, 64, 1.5, -0.5), (16, 4, -0.5, -0.5)])
def test_a_world_moving_with_the_camera_accumulates_like_a_still_one(pt, W, H, k, j):
    still, moved = rigid_pair(pt, W, H, k, j)
    assert_rigid_premise(W, H, still, moved)
    outs = {}
    for name, calls in (("still", still), ("moved", moved)):
        m = mm.MotionTemporalModel(W, H, **tx.OPTS)
        outs[name] = [m.accumulate_scene(*call) for call in calls]
    motion = mm.motion_image(W, H, moved[1][4], moved[0][4], tx.BASIS, moved[1][3])
    assert (motion[..., 3] == 0.0).all() and (motion[..., :3] == U.astype(f32)).all()  # the big sphere, everywhere
    for i in range(2):
        assert same_bits(outs["still"][i][0], outs["moved"][i][0]) and np.array_equal(outs["still"][i][1], outs["moved"][i][1]), i
    kept = outs["still"][1][1] > tx.N
    assert kept.mean() >= 0.7 and not same_bits(outs["still"][1][0], still[1][0])  # (history was found and changed the frame)
    # and the same frames blind to the motion are another result: the motion image is what made them equal
    blind = tm.run_calls(W, H, [c[:4] for c in moved], **tx.OPTS)
    assert not same_bits(blind[0][1], outs["moved"][1][0])


# ---- quality on oracle frames -------------------------------------------------------------------------------------------

MOVING, VELOCITY = 7, (2.5, 0.0, 1.0)


def moving_sequence(oracle, size, frames, spp, ref_spp, pose):
    """Per frame (noisy frame, reference colour, basis, eye, scene): the Cornell box with sphere 7 at constant velocity, the
    generator state carried from frame to frame, each frame's reference at ref_spp from another seed."""
    cornell = oracle.scene_cornell()
    assert cornell["radius"][MOVING] == f32(16.5)  # one of the two object spheres
    state = oracle.setup_random(size, size)
    seq = []
    for k in range(frames):
        eye, yaw = pose(k)
        scene = mm.moved_scene(cornell, {MOVING: VELOCITY}, k)
        basis = oracle.camera_basis(eye, yaw=yaw, w=size, h=size)
        frame = oracle.render(size, size, spp, spheres=scene, basis=basis, eye=eye, rng_state=state)
        ref = oracle.render(size, size, ref_spp, spheres=scene, basis=basis, eye=eye, seed=12345)[..., :3]
        seq.append((frame, ref, basis, np.asarray(eye, f32), scene))
    return seq


def quality(seq, spp, size, **opts):
    """Clamped-colour RMS error of the LAST frame, (whole frame, the moving sphere's pixels) for: no accumulation, accumulation
    blind to the motion, accumulation with motion."""
    blind, aware = tm.TemporalModel(size, size, **opts), mm.MotionTemporalModel(size, size, **opts)
    for frame, ref, basis, eye, scene in seq:
        b, _ = blind.accumulate(frame, spp, basis, eye)
        a, _ = aware.accumulate_scene(frame, spp, basis, eye, scene)
    hit, _, index = mm.first_hit(size, size, scene, basis, eye)
    on = hit & (index == MOVING)
    assert on.sum() >= 0.01 * size * size
    return {name: (fm.clamped_rms(img[..., :3], ref), fm.clamped_rms(img[on][:, :3], ref[on]))
            for name, img in (("none", frame), ("blind", b), ("motion", a))}


def test_model_with_motion_beats_blind_accumulation_and_none_on_the_moving_sphere(oracle):
    """64 x 64 Cornell box, 4 spp, 6 frames, sphere 7 moving by (2.5, 0, 1) per frame, references at 256 spp; the error over the
    pixels whose centre ray hits the moving sphere in the last frame.  Only the ordering is asserted; the figures are printed
    (and recorded in DENOISER.md, "Moving spheres")."""
    seq = moving_sequence(oracle, 64, 6, 4, 256, lambda k: ((50.0, 52.0, 295.6), -90.0))
    q = quality(seq, 4, 64)
    print("QUALITY 64x64 static camera (whole frame, moving sphere):", {k: (round(v[0], 5), round(v[1], 5)) for k, v in q.items()})
    assert q["motion"][1] < q["none"][1]
    assert q["motion"][1] < q["blind"][1]


# ---- the CLI --------------------------------------------------------------------------------------------------------

def _cli(tmp_path, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


VELOCITY_FILES = [
    ("out-of-range", "9 1 0 0\n", ["index 9 outside 0 .. 8"]),
    ("negative-index", "-1 1 0 0\n", ["index -1 outside"]),
    ("repeated", "7 1 0 0\n# again\n7 0 1 0\n", ["line 3", "index 7 is repeated"]),
    ("nan", "7 nan 0 0\n", ["not a finite float"]),
    ("inf", "7 0 inf 0\n", ["not a finite float"]),
    ("beyond-float", "7 0 0 1e39\n", ["not a finite float"]),
    ("three-numbers", "7 1 0\n", ["expected 'index vx vy vz'"]),
    ("five-numbers", "7 1 0 0 0\n", ["expected 'index vx vy vz'"]),
    ("words", "seven 1 0 0\n", ["expected 'index vx vy vz'"]),
    ("fractional-index", "7.5 1 0\n", ["expected 'index vx vy vz'"]),  # (not index 7 moving by (.5, 1, 0))
    ("fractional-index-4", "7.0 1 0 0\n", ["expected 'index vx vy vz'"]),
    ("index-with-tail", "7x 1 0 0\n", ["expected 'index vx vy vz'"]),
    ("empty", "# nothing moves\n\n", ["no velocities"]),
]


@pytest.mark.parametrize("name,text,words", VELOCITY_FILES, ids=[v[0] for v in VELOCITY_FILES])
def test_cli_refuses_a_bad_velocity_file_before_any_device(tmp_path, name, text, words):
    """The device here would fail with a GPUassert line: none of these gets that far."""
    (tmp_path / "v.txt").write_text(text)
    run = _cli(tmp_path, ["--size", "16", "--device", "99", "--frames", "3", "--velocities", "v.txt"])
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: --velocities") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


@pytest.mark.parametrize("args,words", [
    (["--frames", "3", "--velocities", "none.txt"], ["cannot open velocity file none.txt"]),
    (["--poses", "p.txt", "--batch", "--velocities", "v.txt"], ["--velocities cannot be combined with --batch"]),
    (["--progressive", "2", "--velocities", "v.txt"], ["--velocities cannot be combined with --progressive"]),
    (["--velocities", "v.txt"], ["--velocities needs --frames or --poses"]),
    (["--frames", "3", "--spheres", "20", "--velocities", "v20.txt"], ["index 20 outside 0 .. 19"]),
], ids=["unreadable", "with-batch", "with-progressive", "no-frame-loop", "random-scene-range"])
def test_cli_velocity_refusals_come_before_any_device(tmp_path, args, words):
    (tmp_path / "v.txt").write_text("7 1 0 0\n")
    (tmp_path / "v20.txt").write_text("19 1 0 0\n20 1 0 0\n")
    run = _cli(tmp_path, ["--size", "16", "--device", "99"] + args)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


def test_cli_help_lists_the_flag(tmp_path):
    run = _cli(tmp_path, ["--help"])
    assert run.returncode == 0 and "--velocities arg" in run.stdout
