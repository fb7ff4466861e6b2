"""Synthetic three-call sequences for the responsive history of the temporal accumulator (DENOISER.md, "Responsive history"), built
on the helpers of temporal_exact_cases.py: the camera at rest, so every pixel finds itself with one tap of weight 1, and sample
counts 12, 4, 4 with fast_cap 4, so that in the second call tot = 16, k = 1/4 and ftot = 8, kf = 1/2.  A pixel that shall show the
fast colour f and the slow colour x = f - d gets C0 = f - 2 d in the first frame and C1 = f + 2 d in the second:
fC = C0 + (C1 - C0) / 2 = f and C_out = C0 + (C1 - C0) / 4 = f - d, every step exact (asserted in float64).

The probes (second call; clamp_sigma 2).  The window of a probe in a frame corner has m = 4 or 16 taps, so its mean and variance
are dyadic and the expectation is stated by hand -- at the power-of-two size, where a camera at rest reprojects every pixel onto
itself exactly; at the other sizes the fast image is off by a few ulps, so there step 8 is recomputed in scalar arithmetic from the
fast image at hand (scalar_rectify) and the probes that hang on one bit are left to the model.  Everything is held to
tests/temporal_antilag_model.py bit for bit besides.
  corners     a 4 x 4 checkerboard of f = (8 +- 1) / 256 in each corner of the frame: mu = 8/256, var = 1/65536, sigma = 1/256,
              lo = 6/256, hi = 10/256 for the pixel whose window is the block (or its 2 x 2 corner): (0, 0) at R = 1 and 3, (1, 1)
              at R = 2, mirrored.  Top left: channel 0 below lo (-> lo), channel 1 exactly at lo, channel 2 inside: one channel
              clamped, two not.  Top right: above hi (-> hi), exactly at hi, inside.
  constant    a 7 x 7 block of one colour: sigma = 0, the centre is clamped exactly to mu = that colour.
  negative    a 7 x 7 block of one colour with a full mantissa, across columns 31 | 32 and rows 7 | 8, chosen so that
              S2 / m - mu mu < 0 in float32: var = 0.
  nonfinite   the second frame holds NaN at (15, 3) and +Inf at (15, 4), so f and x do: a window with both has NaN bounds and
              passes its centre; a window with the Inf alone has lo = hi = +Inf (the definition's limit); the constant block, more
              than two windows away, clamps.  (The third call then meets them in the history, as step 5 always did.)
  inactive    (16, 20) fails the depth stop in the second call and restarts: tot = ftot = 4, it is not written although its colour
              lies far outside its box."""
import numpy as np

import temporal_exact_cases as tx

f32, f64 = np.float32, np.float64
# (W, H): partial 32 x 8 workgroups on both axes; smaller than the window; one pixel; and a power-of-two size, where reprojection
# at rest is exact (at the others a pixel finds itself with weight 1 - 1e-6 or so: c / H x H is not c in float32)
SIZES = [(37, 19), (3, 2), (1, 1), (64, 32)]
RADII = [1, 2, 3]
SAMPLES = (12, 4, 4)
ANTILAG = dict(fast_cap=4.0, clamp_sigma=2.0)
A, D = 8.0 / 256.0, 1.0 / 256.0
LO, HI = A - 2 * D, A + 2 * D
CONSTANT, CONSTANT_AT = 5.0 / 256.0, (9, 11)
NEGATIVE_AT = (9, 31)
NAN_AT, INF_AT = (15, 3), (15, 4)
INACTIVE_AT = (16, 20)


def window_stats(value, m):
    """(mu, v) of a window of m taps that all hold `value`: the definition's float32 operations, scalar."""
    value = f32(value)
    s1 = s2 = f32(0.0)
    for _ in range(m):
        s1 = f32(s1 + value)
        s2 = f32(s2 + f32(value * value))
    mu = f32(s1 / f32(m))
    return mu, f32(f32(s2 / f32(m)) - f32(mu * mu))


def negative_value(m):
    """A colour in [0.5, 1) whose constant window of m taps has v < 0 by rounding."""
    for i in range(1, 4000):
        value = f32(0.5) + f32(i) * f32(2.0 ** -12) + f32(2.0 ** -23) * f32(i % 7 + 1)
        if window_stats(value, m)[1] < 0:
            return float(value)
    raise AssertionError("no constant with a negative variance found")


def corner_probe(W, H, R, right):
    r = c = 1 if R == 2 else 0
    return (r, W - 1 - c) if right else (r, c)


class Case:
    """calls: [(frame, samples, basis, eye)]; opts: of the session (tx.OPTS and the anti-lag options); f, x: the fast and slow
    colours the second call must form; probes: {name: (row, column)}."""

    def __init__(self, W, H, R):
        self.W, self.H, self.R = W, H, R
        self.name = f"{W}x{H}-R{R}"
        self.exact = W & (W - 1) == 0 and H & (H - 1) == 0
        self.opts = dict(tx.OPTS, clamp_radius=R, **ANTILAG)
        rng = np.random.default_rng(7000 + 100 * W + R)
        f = rng.integers(0, 16, (H, W, 3)) / 256.0
        d = rng.integers(-2, 3, (H, W, 3)) / 256.0
        self.probes = {}
        F = [tx.make_frame(W, H, 7100 + 10 * W + R + i) for i in range(3)]
        if W >= 37 and H >= 19:
            board = np.where((np.add.outer(np.arange(4), np.arange(4)) % 2 == 0)[..., None], A - D, A + D)
            f[0:4, 0:4], f[0:4, W - 4:W] = board, board[:, ::-1]
            tl, tr = corner_probe(W, H, R, False), corner_probe(W, H, R, True)
            # x = f - d: below lo, at lo, inside | above hi, at hi, inside
            d[tl] = f[tl] - np.array([LO - D, LO, A])
            d[tr] = f[tr] - np.array([HI + D, HI, A])
            self.probes.update(below=tl, above=tr)
            (r, c), (rn, cn) = CONSTANT_AT, NEGATIVE_AT
            f[r - 3:r + 4, c - 3:c + 4], d[r, c] = CONSTANT, (2 * D, -3 * D, D)
            self.negative = negative_value((2 * R + 1) ** 2)
            f[rn - 3:rn + 4, cn - 3:cn + 4], d[rn - 3:rn + 4, cn - 3:cn + 4] = self.negative, 0.0
            d[rn, cn] = 2.0 ** -16
            self.probes.update(constant=CONSTANT_AT, negative=NEGATIVE_AT, nan=NAN_AT, inf=INF_AT, inactive=INACTIVE_AT)
            d[NAN_AT[0] - 3:NAN_AT[0] + 4, 0:INF_AT[1] + 5] = 3 * D  # (whoever keeps a finite box around here lies outside it)
        C0, C1 = f - 2 * d, f + 2 * d
        assert tx.is_f32(C0) and tx.is_f32(C1) and tx.is_f32(f) and tx.is_f32(f - d)
        assert np.array_equal(C0 + (C1 - C0) / 2, f) and np.array_equal(C0 + (C1 - C0) / 4, f - d) and tx.is_f32(C1 - C0)
        F[0][..., 0:3], F[1][..., 0:3] = C0, C1
        self.f, self.x = f.astype(f32), (f - d).astype(f32)
        if "nan" in self.probes:
            F[1][NAN_AT][0:3], F[1][INF_AT][0:3] = np.nan, np.inf  # (the second frame alone: Inf - Inf would be another NaN)
            self.f[NAN_AT], self.x[NAN_AT], self.f[INF_AT], self.x[INF_AT] = np.nan, np.nan, np.inf, np.inf
            F[1][INACTIVE_AT][9] = 64.0  # fails the depth stop against the history's 8
            F[1][INACTIVE_AT][0:3] = 200.0 / 256.0
            self.f[INACTIVE_AT] = self.x[INACTIVE_AT] = 200.0 / 256.0
        self.calls = [(np.ascontiguousarray(Fi, f32), n, tx.BASIS, tx.EYE.astype(f32)) for Fi, n in zip(F, SAMPLES)]
        for Fi, _, _, _ in self.calls:
            Fi.setflags(write=False)

    def __repr__(self):
        return self.name


def scalar_rectify(fast, x, r, c, R, k, tot):
    """Step 8 for ONE pixel in scalar float32, one statement per operation: (y[3], active, m)."""
    H, W = fast.shape[:2]
    y = []
    for ch in range(3):
        m = s1 = s2 = f32(0.0)
        for tr in range(r - R, r + R + 1):
            for tc in range(c - R, c + R + 1):
                if 0 <= tr < H and 0 <= tc < W:
                    t = f32(fast[tr, tc, ch])
                    m = f32(m + f32(1.0))
                    s1 = f32(s1 + t)
                    s2 = f32(s2 + f32(t * t))
        mu = f32(s1 / m)
        v = f32(f32(s2 / m) - f32(mu * mu))
        sd = f32(f32(k) * f32(np.sqrt(v if v > 0 else f32(0.0))))
        lo, hi = f32(mu - sd), f32(mu + sd)
        xc = f32(x[r, c, ch])
        y.append(lo if xc < lo else (hi if xc > hi else xc))
    active = bool(f32(tot) > f32(fast[r, c, 3]))
    return np.array(y if active else x[r, c], f32), active, int(m)


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_second_call(case, out, counts, fast, x, what):
    """What the second call must give.  out [H][W][14], counts [H][W] and fast [H][W][4] from the model or from the kernel; x
    [H][W][3]: the colour step 7 formed, before step 8 (the model's: the kernel does not show it).
    Every size: counts and fast counts; the channels the stage must not touch; step 8 again in scalar arithmetic, from the given
    fast image, at every probe, every corner, the middle of every edge and the pixels around the workgroup borders; the probes
    that do not hang on the last bit (below lo, above hi, the constant block, the NaN's window, the Inf's, the inactive pixel).
    Power-of-two sizes, where reprojection at rest is exact (temporal_exact_cases.py): the fast image, x and every probe stated
    by hand -- exactly at lo and at hi, sigma = 0, the negative variance."""
    with np.errstate(all="ignore"):
        _check_second_call(case, out, counts, fast, x, what)


def _check_second_call(case, out, counts, fast, x, what):
    H, W, R = case.H, case.W, case.R
    tag = (what, case.name)
    p = case.probes
    restarted = np.zeros((H, W), bool)
    if p:
        restarted[p["inactive"]] = True
    assert np.array_equal(fast[..., 3], np.where(restarted, 4.0, 8.0)) and np.array_equal(counts, np.where(restarted, 4, 16)), tag
    F1 = case.calls[1][0]
    assert _same(out[..., 3:10], F1[..., 3:10]) and _same(out[..., 11:], F1[..., 11:]), tag
    y = out[..., 0:3]
    spots = {(r, c) for r in (0, H // 2, H - 1) for c in (0, W // 2, W - 1)} | set(p.values())
    spots |= {(r, c) for r in (7, 8) for c in (31, 32) if r < H and c < W}
    for r, c in sorted(spots):
        tot = 4.0 if restarted[r, c] else 16.0
        want, active, m = scalar_rectify(fast, x, r, c, R, ANTILAG["clamp_sigma"], tot)
        assert _same(y[r, c], want), (tag, r, c, y[r, c], want)
        assert active != restarted[r, c]
        assert m == (min(r + R, H - 1) - max(r - R, 0) + 1) * (min(c + R, W - 1) - max(c - R, 0) + 1)
    if (W, H) == (1, 1):  # m = 1: mu = f, v = f f - f f = 0: clamped to the fast colour
        assert _same(y, fast[..., 0:3]), tag
    if not p:
        return
    below, above = p["below"], p["above"]
    assert x[below][0] < y[below][0] < A and x[above][0] > y[above][0] > A, (tag, "one channel is clamped")
    assert y[below][2] == x[below][2] and y[above][2] == x[above][2], (tag, "and another one is not")
    for at in ((NAN_AT[0] + 1, NAN_AT[1]), (NAN_AT[0] + 1, NAN_AT[1] + 1)):  # the NaN's window passes what a finite box would clamp
        assert _same(y[at], x[at]) and np.isfinite(y[at]).all(), (tag, at)
    assert np.isnan(y[NAN_AT]).all() and np.isposinf(y[INF_AT]).all()
    alone = (INF_AT[0] + R, INF_AT[1] + R)  # the Inf in the window's corner, without any NaN
    assert np.isposinf(y[alone]).all() and np.isfinite(x[alone]).all(), (tag, y[alone])
    assert _same(y[p["inactive"]], F1[p["inactive"]][0:3]) and not restarted.all(), tag
    assert abs(y[p["constant"]] - f32(CONSTANT)).max() < D / 64 < abs(x[p["constant"]] - f32(CONSTANT)).min(), (tag, "far from the NaN")
    if not case.exact:
        return
    assert _same(fast[..., 0:3], case.f) and _same(x, case.x), tag
    assert y[below].tolist() == [LO, LO, A] and x[below].tolist() == [LO - D, LO, A], (tag, y[below])
    assert y[above].tolist() == [HI, HI, A] and x[above].tolist() == [HI + D, HI, A], (tag, y[above])
    assert y[p["constant"]].tolist() == [CONSTANT] * 3 and not (x[p["constant"]] == f32(CONSTANT)).any(), (tag, y[p["constant"]])
    mu, v = window_stats(case.negative, (2 * R + 1) ** 2)
    assert v < 0 and x[p["negative"]][0] != mu and y[p["negative"]].tolist() == [float(mu)] * 3, (tag, y[p["negative"]], mu, v)


CASES = [Case(W, H, R) for W, H in SIZES for R in RADII]
