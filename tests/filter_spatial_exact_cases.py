"""Exact cases of the feature filter's spatial variance estimate, shared by test_filter_spatial_exact_host.py (the float32 model
against closed forms, on the CPU) and test_filter_spatial_exact_gpu.py (the kernel against both).

Built like tests/filter_exact_cases.py: the demodulator is 2^-8, so the set-up only moves exponents; the stops are open (sigma
1e30) or the normal stop is closed between classes (one-hot normals, sigma_n 2^-10), so that every weight is exactly 1 or 0.
The luminance is made an integer: only the green channel is lit, with the float32 g for which 0.7152f x g rounds to AMP exactly
(found by search, asserted), so L is AMP on a lattice of `lit` pixels and 0 elsewhere.  A window with N admitted taps of which k
are lit then has, in integers,
    m = k AMP / N,   sum w (L - m)^2 = AMP^2 k (N - k) / N =: S,   v = S / N
and wherever N divides k AMP and AMP^2 k (N - k) / N < 2^24 every product, difference and partial sum is an integer below 2^24:
exact in float32 in any order, with or without contraction, and v is the one rounding of an IEEE quotient.  AMP is a common
multiple of the window sizes that occur, the lattice has the window's pitch 2R + 1 and starts at pixel (0, 0), and the frame
sizes put lattice points on every edge and corner; workgroup borders (x = 31 | 32, y = 7 | 8) lie inside every frame.  Where
the condition fails (R = 3, some corner windows) `exact` is False and only the float32 model's bits are asked for."""
import functools

import numpy as np

import filter_exact_cases as fx
import filter_model as fm

N = fx.N
OPEN = fx.OPEN
GREEN = np.float32(0.7152)
SIZES = {1: (67, 19), 2: (66, 21), 3: (64, 22)}  # (w, h) = multiples of 2R + 1, plus 1: more than one workgroup each way
# R = 1: windows of 4, 6, 9 taps; R = 2: 9 .. 25 (lcm 3600); R = 3: 2940 = lcm(28, 35, 42, 49) for the interior and the edges,
# 3600 = lcm(16, 20, 24, 25, 30, 36) at the lattice points of the four corners
AMP = {1: 36, 2: 3600, 3: 2940}
CORNER_AMP = {1: 36, 2: 3600, 3: 3600}
KINDS = ("open", "normal")


def green_for(level):
    """The float32 g with float32(0.7152f x g) == level."""
    g0 = np.float32(np.float64(level) / np.float64(GREEN))
    for step in range(-4, 5):
        g = g0
        for _ in range(abs(step)):
            g = np.nextafter(g, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
        if np.float32(GREEN * g) == np.float32(level):
            return g
    raise AssertionError(f"no float32 green gives luminance {level}")


@functools.lru_cache(maxsize=None)
def case(kind, radius):
    """-> dict(frame, sigmas, cls, amp [H][W] int64 (0 where unlit), var0 [H][W] float32 (the set-up's variance))."""
    w, h = SIZES[radius]
    d = 2 * radius + 1
    rng = np.random.default_rng([radius, KINDS.index(kind)])
    ys, xs = np.mgrid[0:h, 0:w]
    lit = (ys % d == 0) & (xs % d == 0)
    corner = ((ys == 0) | (ys == h - 1)) & ((xs == 0) | (xs == w - 1))
    assert lit[0, 0] and lit[h - 1, w - 1] and lit[0, w - 1] and lit[h - 1, 0]
    amp = np.where(lit, np.where(corner, CORNER_AMP[radius], AMP[radius]), 0).astype(np.int64)
    ill = np.zeros((h, w, 3), np.float32)
    for level in np.unique(amp[amp > 0]):
        ill[amp == level, 1] = green_for(int(level))
    var = rng.integers(1, 9, (h, w))
    sigmas = dict(OPEN)
    cls = np.zeros((h, w), np.int64)
    v = rng.normal(size=(h, w, 3))
    normals = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    if kind == "normal":
        sigmas.update(fx.STOPS["normal"][0])
        cls = fx.bands(w, h, 3)
        normals = np.eye(3, dtype=np.float32)[cls]
    depth = (1.0 + xs + 2.0 * ys).astype(np.float32)
    a = np.float32(2.0 ** -8)
    f = np.zeros((h, w, 14), np.float32)
    f[..., 0:3] = ill * a
    f[..., 3:6] = normals
    f[..., 6:9] = np.float32(a - fm.EPS32)
    f[..., 9] = depth
    f[..., 10] = var.astype(np.float32) * np.float32(N) * a * a
    assert np.float32(fm.EPS32 + f[0, 0, 6]) == a
    ill32, var0, _, _ = fm.setup(f, samples=N, dtype=np.float32)
    assert np.array_equal(fm._lum(np.float32, ill32), amp.astype(np.float32))  # the luminance IS the integer image
    assert np.array_equal(var0, var.astype(np.float32))
    out = dict(frame=f, sigmas=sigmas, cls=cls, amp=amp, var0=var0, radius=radius)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def closed_form(c, poison=None):
    """-> (v [H][W] float32, exact [H][W] bool, taps [H][W]): the closed form of the estimate wherever it is exact, over "in the
    frame and of the pixel's class".  poison (y, x): that pixel is non-finite, so every pixel with it as an in-frame tap has a
    NaN estimate (of whatever class: 0 x NaN is NaN); such pixels come back as NaN, exact."""
    cls, amp, R = c["cls"], c["amp"], c["radius"]
    h, w = cls.shape
    n, s1, s2 = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    reach = np.zeros((h, w), bool)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            y0, y1, x0, x1 = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
            if y0 >= y1 or x0 >= x1:
                continue
            p, q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + j, y1 + j), slice(x0 + i, x1 + i))
            ok = (cls[q] == cls[p]).astype(np.int64)
            n[p] += ok
            s1[p] += ok * amp[q]
            s2[p] += ok * amp[q] * amp[q]
            if poison is not None:
                hit = np.zeros((h, w), bool)
                hit[poison] = True
                reach[p] |= hit[q]
    # sum (L - m)^2 = s2 - s1^2 / n; with one amplitude A and k lit taps: A^2 k (n - k) / n
    exact = (s1 % n == 0) & ((s1 * s1) % n == 0)
    S = s2 - (s1 * s1) // n
    m = s1 // n
    worst = np.maximum(S, (np.max(amp) - np.minimum(m, np.max(amp))) ** 2)
    exact &= (worst < 2 ** 24) & (S >= 0)
    v = (S.astype(np.float64) / n.astype(np.float64)).astype(np.float32)  # (float64 quotient of two float32 integers: one rounding)
    v = np.where(reach, np.float32(np.nan), v)
    return v, exact | reach, n


POISON_AT = {1: {"corner": (0, 0), "left": (9, 0), "top": (0, 33), "border": (8, 32), "last": (18, 66)},
             2: {"corner": (0, 0), "left": (10, 0), "top": (0, 30), "border": (8, 32), "last": (20, 65)},
             3: {"corner": (0, 0), "left": (7, 0), "top": (0, 35), "border": (8, 32), "last": (21, 63)}}  # (y, x)


def poisoned(c, where, value):
    f = c["frame"].copy()
    y, x = POISON_AT[c["radius"]][where]
    f[y, x, 0:3] = value
    return f, (y, x)
