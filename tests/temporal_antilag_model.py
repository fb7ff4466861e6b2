"""NumPy restatement of the temporal accumulator's responsive history (include/ptcore.h, pt_temporal_set_antilag and
pt_temporal_fast; DENOISER.md, "Temporal accumulation", "Responsive history"), for the tests and tools/temporal_antilag_quality.py.
Float32, one rounding per operation, in the order the definition writes them.

Neither temporal_model.py nor temporal_motion_model.py is copied.  Steps 5f and 6f use the same four taps, `valid` and weights as
step 5, and TemporalModel._gather forms exactly those sums for whatever stands in the first history image: so the fast history is
gathered by a second call of the inherited _gather with {fC, fn} standing where {colour, s2} stand (its `hs2` is then
sum(w fn') / Ws, selected to 0 without history).  Step 8 is written out here: a loop over the (2R+1)^2 offsets in row-major order."""
import numpy as np

import temporal_motion_model as tmm

f32 = np.float32
DEFAULT_SIGMA, DEFAULT_RADIUS = 1.0, 1  # PT_ANTILAG_DEFAULT_SIGMA, PT_ANTILAG_DEFAULT_RADIUS (include/ptcore.h)


def check_antilag(fast_cap, clamp_sigma, clamp_radius, history_cap, reserved=0):
    """The host checks of pt_temporal_set_antilag: ValueError naming the field for what the C ABI refuses."""
    fast_cap, clamp_sigma, history_cap = f32(fast_cap), f32(clamp_sigma), f32(history_cap)
    if fast_cap != 0 and not (fast_cap >= 1 and fast_cap < history_cap):
        raise ValueError("fast_cap")
    if not (clamp_sigma > 0 and np.isfinite(clamp_sigma)):
        raise ValueError("clamp_sigma")
    if int(clamp_radius) != clamp_radius or not 1 <= clamp_radius <= 3:
        raise ValueError("clamp_radius")
    if reserved != 0:
        raise ValueError("reserved")


class AntilagTemporalModel(tmm.MotionTemporalModel):
    """MotionTemporalModel with a fast history.  fast_cap = 0 is MotionTemporalModel itself.  After every call `fast` holds
    [H][W][4] {fC, ftot} (pt_temporal_fast) and `last` what step 8 saw (None when it was not issued)."""

    def __init__(self, width, height, fast_cap=0.0, clamp_sigma=DEFAULT_SIGMA, clamp_radius=DEFAULT_RADIUS, **opts):
        super().__init__(width, height, **opts)
        self.fast_cap, self.k, self.R = f32(0.0), f32(DEFAULT_SIGMA), DEFAULT_RADIUS
        self.fast = self.last = self._fh = None
        self.set_antilag(fast_cap, clamp_sigma, clamp_radius)

    def set_antilag(self, fast_cap, clamp_sigma=DEFAULT_SIGMA, clamp_radius=DEFAULT_RADIUS):
        check_antilag(fast_cap, clamp_sigma, clamp_radius, self.cap)
        if self.hist is not None:
            raise ValueError("reset the session")
        self.fast_cap, self.k, self.R = f32(fast_cap), f32(clamp_sigma), int(clamp_radius)
        self.fast = self.last = None

    def reset(self):
        super().reset()
        self.fast = self.last = None

    def _gather(self, C, N, A, z, basis, eye):
        slow = super()._gather(C, N, A, z, basis, eye)
        if self.fast_cap > 0:  # 5f: the same taps, validity and weights over the fast image
            hist = self.hist
            self.hist = (self.fast, hist[1], hist[2])
            try:
                fhC, fhn, _ = super()._gather(C, N, A, z, basis, eye)
            finally:
                self.hist = hist
            self._fh = (fhC, np.fmin(fhn, self.fast_cap))
        return slow

    def accumulate(self, frame, n, basis, eye, motion=None, _keep_scene=False):
        if not self.fast_cap > 0:
            return super().accumulate(frame, n, basis, eye, motion, _keep_scene)
        H, W = self.H, self.W
        had_history = self.hist is not None
        self._fh, self.last = None, None
        out, counts = super().accumulate(frame, n, basis, eye, motion, _keep_scene)
        C = np.array(frame, dtype=f32).reshape(H, W, 14)[..., 0:3]
        fhC, fhN = self._fh if had_history else (np.zeros((H, W, 3), f32), np.zeros((H, W), f32))
        with np.errstate(all="ignore"):  # 6f
            ftot = fhN + f32(n)
            kf = f32(n) / ftot
            fC = fhC + kf[..., None] * (C - fhC)
        assert fC.dtype == f32 and ftot.dtype == f32
        self.fast = np.concatenate([fC, ftot[..., None]], -1)
        if had_history:
            self._rectify(out)
        return out, counts

    def _rectify(self, out):
        """Step 8, on the frame `out` and the slow history that step 7 just wrote."""
        H, W, R = self.H, self.W, self.R
        fC, ftot = self.fast[..., 0:3], self.fast[..., 3]
        tot = self.hist[2][..., 3]
        rows, cols = np.mgrid[0:H, 0:W]
        m = np.zeros((H, W), f32)
        S1, S2 = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
        with np.errstate(all="ignore"):
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    tr, tc = rows + dy, cols + dx
                    inside = (tr >= 0) & (tr < H) & (tc >= 0) & (tc < W)
                    x = fC[np.clip(tr, 0, H - 1), np.clip(tc, 0, W - 1)]
                    m = np.where(inside, m + f32(1.0), m)
                    S1 = np.where(inside[..., None], S1 + x, S1)
                    S2 = np.where(inside[..., None], S2 + x * x, S2)
            mu = S1 / m[..., None]
            v = S2 / m[..., None] - mu * mu
            var = np.where(v > 0, v, f32(0.0))
            sd = self.k * np.sqrt(var)
            lo, hi = mu - sd, mu + sd
            x = self.hist[0][..., 0:3]
            y = np.where(x < lo, lo, np.where(x > hi, hi, x))
        active = tot > ftot
        y = np.where(active[..., None], y, x)
        for a in (m, S1, S2, mu, v, var, sd, lo, hi, y):
            assert a.dtype == f32
        self.last = dict(m=m, mu=mu, v=v, var=var, lo=lo, hi=hi, active=active, x=x.copy(), y=y)
        out[..., 0:3] = y
        self.hist[0][..., 0:3] = y


def run_calls(width, height, calls, **opts):
    """calls [(frame, samples, basis, eye)] through one session: ([frame after the stage], [counts], [fast image], [last])."""
    m = AntilagTemporalModel(width, height, **opts)
    outs, counts, fasts, lasts = [], [], [], []
    for f, n, b, e in calls:
        o, c = m.accumulate(f, n, b, e)
        outs.append(o), counts.append(c), fasts.append(None if m.fast is None else m.fast.copy()), lasts.append(m.last)
    return outs, counts, fasts, lasts


def accumulate_scenes(frames, n, bases, eyes, scenes, **opts):
    """A sequence through one _scene session: (frames after the stage [K][H][W][14], counts [K][H][W], fast images [K][H][W][4]
    or None with anti-lag off)."""
    frames = np.asarray(frames, dtype=f32)
    m = AntilagTemporalModel(frames.shape[2], frames.shape[1], **opts)
    outs, counts, fasts = [], [], []
    for f, b, e, s in zip(frames, bases, eyes, scenes):
        o, c = m.accumulate_scene(f, n, b, e, s)
        outs.append(o), counts.append(c), fasts.append(None if m.fast is None else m.fast.copy())
    return np.stack(outs), np.stack(counts), (np.stack(fasts) if fasts[0] is not None else None)


# ---- the lamp sequence (DENOISER.md, "Responsive history"): light that moves ---------------------------------------------------
LAMP_INDEX = 8  # the Cornell box's ceiling light, replaced by a lamp inside the room
# the lamp hangs near the camera and crosses the view: its disc moves a long way per frame, its light on the far walls changes
# gently -- most static surfaces keep a stable light, the ones near the lamp do not.  HARD_LAMP is the scene of the recorded
# limit: a lamp deep in the room that sweeps through it, so that ALL light moves by several times the references' noise.
LAMP = dict(radius=16.0, pos=(14.0, 45.0, 180.0), emission=(1.25, 1.125, 1.0), step=(6.5, 0.0, 0.0))
HARD_LAMP = dict(radius=30.0, pos=(25.0, 45.0, 25.0), emission=(1.5, 1.35, 1.2), step=(5.0, 0.0, 13.0))


def lamp_scene(cornell, k):
    """The scene of frame k: sphere 8 is an emitting sphere (LAMP) at pos + (float)k * step per component in float32."""
    s = np.array(cornell, copy=True)
    s["radius"][LAMP_INDEX], s["emission"][LAMP_INDEX], s["color"][LAMP_INDEX] = LAMP["radius"], LAMP["emission"], 0.0
    s["pos"][LAMP_INDEX] = np.asarray(LAMP["pos"], f32) + f32(k) * np.asarray(LAMP["step"], f32)
    return s


def static_mask(width, height, scene, basis, eye):
    """The pixels whose centre ray hits a sphere that does not move: every hit but the lamp's."""
    hit, _, index = tmm.first_hit(width, height, scene, basis, eye)
    return hit & (index != LAMP_INDEX)
