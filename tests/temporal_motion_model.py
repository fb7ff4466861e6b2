"""NumPy restatement of temporal accumulation with per-pixel motion (include/ptcore.h, pt_temporal_motion and the _motion / _scene
calls; DENOISER.md, "Temporal accumulation", "Moving spheres"), for the tests.  Two pieces, both float32 operation by operation:

  motion_image     the motion kernel: the unjittered primary ray of every pixel (numpy_restatement._primary), the reference's
                   nearest-hit search (numpy_restatement.intersect_scene), m = pos_now[i] - pos_prev[i], w = (float)i; a miss is
                   (0, 0, 0, -1).
  MotionTemporalModel  temporal_model.TemporalModel with the ONE extra subtraction Xp = X - m in front of X - eye'.

Neither temporal_model.py nor numpy_restatement.py is copied: TemporalModel._gather forms `X[k] - self.eye[k]`, and for the call
with a motion image self.eye[k] is an object whose reflected subtraction is (X[k] - m[k]) - eye'[k]."""
import numpy as np

import numpy_restatement as nr
import temporal_model as tm

f32 = np.float32
MOTION_CHUNK = 256  # PT_MOTION_CHUNK (include/ptcore.h): spheres staged per round of the motion kernel


def check_scenes(now, prev):
    """The host checks of pt_temporal_motion: ValueError for what the C ABI refuses."""
    if len(now) != len(prev) or not 1 <= len(now) <= 65535:
        raise ValueError("n")
    for s in (now, prev):
        for field in ("radius", "pos", "emission", "color"):
            if not np.isfinite(s[field]).all():
                raise ValueError("not finite")
    if not np.array_equal(now["radius"].view(np.uint32), prev["radius"].view(np.uint32)):
        raise ValueError("radius: reset the session")


def first_hit(width, height, spheres, basis, eye):
    """(hit, t, index) of the centre ray of every pixel, the reference's arithmetic."""
    o, d = nr._primary(width, height, basis, eye)
    return nr.intersect_scene(o, d, spheres)


def motion_image(width, height, spheres_now, spheres_prev, basis, eye):
    """float32 [H][W][4] {mx, my, mz, w}."""
    check_scenes(spheres_now, spheres_prev)
    tm.camera_matrix(basis)  # (the refusals of the camera step)
    hit, _, index = first_hit(width, height, spheres_now, basis, eye)
    now, prev = np.asarray(spheres_now["pos"], f32), np.asarray(spheres_prev["pos"], f32)
    delta = now - prev  # one float32 subtraction per component
    out = np.zeros((height, width, 4), f32)
    out[..., :3] = np.where(hit[..., None], delta[index], f32(0.0))
    out[..., 3] = np.where(hit, index.astype(f32), f32(-1.0))
    return out


class _Moved:
    """Stands where TemporalModel keeps one component of the previous eye: X - this = (X - m) - eye'."""
    __array_ufunc__ = None  # ndarray.__sub__ defers to __rsub__

    def __init__(self, m, e):
        self.m, self.e = m, e

    def __rsub__(self, X):
        Xp = X - self.m
        assert Xp.dtype == f32
        return Xp - self.e


class MotionTemporalModel(tm.TemporalModel):
    """accumulate(frame, n, basis, eye, motion=None): motion is [H][W][4] (or [..., :3]); None is the static call.
    accumulate_scene(frame, n, basis, eye, spheres): the _scene session."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.scene = None

    def reset(self):
        super().reset()
        self.scene = None

    def accumulate(self, frame, n, basis, eye, motion=None, _keep_scene=False):
        if not _keep_scene:
            self.scene = None  # a plain call forgets the remembered scene
        if motion is not None and self.hist is not None:
            m = np.asarray(motion, f32).reshape(self.H, self.W, -1)
            self.eye = [_Moved(m[..., k], self.eye[k]) for k in range(3)]
        return super().accumulate(frame, n, basis, eye)  # (which leaves the plain eye of this call behind)

    def accumulate_scene(self, frame, n, basis, eye, spheres):
        spheres = np.array(spheres, copy=True)
        motion = None
        if self.hist is not None and self.scene is not None:
            motion = motion_image(self.W, self.H, spheres, self.scene, basis, eye)
        elif self.hist is not None:
            check_scenes(spheres, spheres)
        out = self.accumulate(frame, n, basis, eye, motion, _keep_scene=True)
        self.scene = spheres
        return out


def accumulate_scenes(frames, n, bases, eyes, scenes, **opts):
    """A sequence through one _scene session: (frames after the stage [K][H][W][14], counts [K][H][W])."""
    frames = np.asarray(frames, dtype=f32)
    m = MotionTemporalModel(frames.shape[2], frames.shape[1], **opts)
    outs, counts = zip(*(m.accumulate_scene(f, n, b, e, s) for f, b, e, s in zip(frames, bases, eyes, scenes)))
    return np.stack(outs), np.stack(counts)


def moved_scene(spheres, velocities, k):
    """The scene of frame k of `pathtrace --velocities`: centre pos0 + (float)k * v per component in float32."""
    s = np.array(spheres, copy=True)
    for index, v in velocities.items():
        s["pos"][index] = s["pos"][index] + f32(k) * np.asarray(v, f32)
    return s
