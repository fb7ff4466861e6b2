"""Exact cases of the feature-guided filter, shared by test_filter_exact_host.py (the NumPy model against hand-worked
expectations, on the CPU) and test_filter_exact_gpu.py (the kernel against both).

Frames are built from integers: illumination `ill` (integers through a demodulator a = EPS + albedo that is a power of two),
variance `var` (integers: channel 10 = var x n x a^2) -- so the set-up is exact by construction -- and a class image `cls`.
With one stop at a sigma so small that a tap of another class is refused outright, and the other three at 1e30, a tap's
weight is the dyadic h = k[i] k[j] (exponent 0) or 0, and one iteration is the exact dyadic mean over "in the frame and of
the pixel's class".  exact_step() computes that mean in integer arithmetic on slices of the images, without the model."""
import functools
import os

import numpy as np

import filter_model as fm
from conftest import GOLDEN

SIZES = ((37, 29), (64, 64), (33, 9))  # (w, h); 33 x 9: one column into a second workgroup of 32 x 8, one row into a second
STEPS = (1, 2, 4, 8, 16)
N = 4                                   # the uniform count of the built frames
OPEN = dict(sigma_l=1e30, sigma_n=1e30, sigma_a=1e30, sigma_z=1e30)
HN = (1, 4, 6, 4, 1)                    # 16 x the a-trous kernel
STOPS = {  # stop -> (the sigma that closes it, number of classes, floor of a refused tap's exponent)
    "normal": (dict(sigma_n=2.0 ** -10), 3, 1000.0),  # |e_a - e_b|^2 = 2 over 2^-20
    "albedo": (dict(sigma_a=2.0 ** -20), 2, 1000.0),  # 3 x (2^-9)^2 over 2^-40
    # depth: plateaus 8, 72, 136, and the definition's 1e-3 |z_p| in the denominator: the nearest other plateau of the farthest
    # one is 64 / 0.136 = 470.6 away (three depths on a line cannot all be farther from each other than from 0: below 1000
    # for any choice).  The float32 exponential is 0 there; the float64 one is 1e-205, which no sum here can hold.
    "depth": (dict(sigma_z=2.0 ** -30), 3, 470.0),
    # luminance: 1 against 65, and the definition's 0.01 |L_p|: 64 / 0.6501 = 98.4 seen from the bright side (below 100 for any
    # two positive luminances).  A weight of h e^-98 = h 2e-43 is absorbed by every sum it enters (all are >= 9/64, or sums
    # of luminances >= 1), in float32 and in float64.
    "luminance": (dict(sigma_l=2.0 ** -40), 2, 98.0),
}
GOLDEN_FRAMES = (("oracle_64_spp1_xorwow", 1), ("oracle_64_spp4_xorwow", 4), ("oracle_64_spp16_xorwow_glm_b8", 16))
SHAPES = {"64x64": (slice(0, 64), slice(0, 64)), "29x37": (slice(17, 46), slice(11, 48)), "5x64": (slice(30, 35), slice(0, 64)),
          "64x3": (slice(0, 64), slice(40, 43)), "1x1": (slice(16, 17), slice(59, 60))}  # (test_filter_gpu.py's crops)
COUNT_VALUES = (0, 1, 2, 40, 2 ** 32 - 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bands(w, h, m):
    """Slanted bands 2 to 4 pixels wide: every 5 x 5 neighbourhood holds more than one class."""
    y, x = np.mgrid[0:h, 0:w]
    return ((3 * x + 5 * y) // 11) % m


def build_frame(ill, var, a_log2, normals, depth):
    """The frame whose set-up is exactly (ill, var) with the demodulator 2^a_log2: integers in, float32 [H][W][14] out."""
    h, w = var.shape
    a = np.exp2(a_log2.astype(np.float64)).astype(np.float32)
    alb = (a - fm.EPS32).astype(np.float32)
    # EPS + albedo is the power of two in both precisions (2^-8 and 2^-9 are; 2^-7 - EPS is no float32)
    assert np.array_equal(fm.EPS32 + alb, a) and np.array_equal(np.float64(fm.EPS32) + alb.astype(np.float64), a.astype(np.float64))
    f = np.zeros((h, w, 14), np.float32)
    f[..., 0:3] = ill.astype(np.float32) * a[..., None]
    f[..., 3:6] = normals
    f[..., 6:9] = alb[..., None]
    f[..., 9] = depth
    f[..., 10] = var.astype(np.float32) * np.float32(N) * a * a
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def case(kind, w, h):
    """kind: "open" (all four stops open), a key of STOPS (that stop closed between classes), or "chain" (open, 0 / 1 images for
    the chains of steps).  Returns a dict: frame, sigmas, cls, ill [H][W][3] and var [H][W] (int64, the exact set-up)."""
    rng = np.random.default_rng([w, h, sorted(list(STOPS) + ["open", "chain"]).index(kind)])
    ill = rng.integers(0, 16, (h, w, 3))
    var = rng.integers(1, 9, (h, w))
    v = rng.normal(size=(h, w, 3))
    normals = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    depth = (1.0 + np.arange(w)[None, :] + 2.0 * np.arange(h)[:, None]).astype(np.float32)
    a_log2 = np.full((h, w), -8)
    cls = np.zeros((h, w), np.int64)
    sigmas = dict(OPEN)
    if kind in STOPS:
        closed, m, _ = STOPS[kind]
        sigmas.update(closed)
        cls = bands(w, h, m)
    if kind == "normal":
        normals = np.eye(3, dtype=np.float32)[cls]
    elif kind == "albedo":
        a_log2 = -8 - cls
    elif kind == "depth":
        depth = (8.0 + 64.0 * cls).astype(np.float32)
    elif kind == "luminance":
        ill = np.repeat((1 + 64 * cls)[..., None], 3, axis=-1)
    elif kind == "chain":
        # var 1 on a lattice of spacing 3 (and the last row and column), so that every 3 x 3 blur is positive and sigma_l = 1e30
        # keeps the luminance stop open (with sd = 0 its denominator would be 0.01 |L| + 1e-4), and 1 at an eighth of the other
        # pixels: sparse, so that two iterations' integer numerators stay below 2^24
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        lattice = ((ys % 3 == 0) | (ys == h - 1)) & ((xs % 3 == 0) | (xs == w - 1))
        ill, var = rng.integers(0, 2, (h, w, 3)), (lattice | (rng.integers(0, 8, (h, w)) == 0)).astype(np.int64)
    out = dict(frame=build_frame(ill, var, a_log2, normals, depth), sigmas=sigmas, cls=cls, ill=ill.astype(np.int64),
               var=var.astype(np.int64), a=np.exp2(a_log2.astype(np.float64)).astype(np.float32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exact_step(ill, var, cls, step):
    """One iteration over "in the frame and of the pixel's class" in integers: (SI [H][W][3], SV [H][W], SW [H][W], admitted,
    refused) with ill' = SI / SW, var' = SV / SW^2 (SW = 256 x the sum of the weights), and per pixel the numbers of admitted
    and of refused off-centre taps inside the frame."""
    h, w = cls.shape
    si, sv, sw = np.zeros((h, w, 3), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    admitted, refused = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for j in range(-2, 3):
        for i in range(-2, 3):
            y0, y1, x0, x1 = max(0, -j * step), min(h, h - j * step), max(0, -i * step), min(w, w - i * step)
            if y0 >= y1 or x0 >= x1:
                continue
            p = (slice(y0, y1), slice(x0, x1))
            q = (slice(y0 + j * step, y1 + j * step), slice(x0 + i * step, x1 + i * step))
            ok = (cls[q] == cls[p]).astype(np.int64)
            hn = HN[i + 2] * HN[j + 2]
            sw[p] += hn * ok
            si[p] += (hn * ok)[..., None] * ill[q]
            sv[p] += hn * hn * ok * var[q]
            if i or j:
                admitted[p] += ok
                refused[p] += 1 - ok
    return si, sv, sw, admitted, refused


def rounded_quotient(num, den):
    """The float32 nearest num / den for integer images below 2^24: both are float32 values, so the float64 quotient rounds to
    the float32 one without a double-rounding error (53 >= 2 x 24 + 2)."""
    assert (0 <= num).all() and (num < 2 ** 24).all() and (0 < den).all() and (den < 2 ** 24).all()
    return (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)


def expected_step(c, step):
    """case -> (ill' [H][W][3], var' [H][W]) float32 after ONE iteration at `step`, and the admitted / refused counts."""
    si, sv, sw, admitted, refused = exact_step(c["ill"], c["var"], c["cls"], step)
    return rounded_quotient(si, np.broadcast_to(sw[..., None], si.shape)), rounded_quotient(sv, sw * sw), admitted, refused


def expected_chain(c, steps):
    """case "chain" -> (ill [H][W][3], var [H][W] or None, margin): the state after the unfused iterations `steps`, exact
    where all their taps lie inside the frame, that is `margin` = 2 x sum(steps) pixels from every border: there the sum of the
    weights is 1, every state is a dyadic rational (ill a multiple of 2^-8k below 1, var of 2^-16k) and every float32 sum of
    the kernel is exact as long as the integer numerators stay below 2^24.  var is None when they do not."""
    ill, var, k, margin = c["ill"], c["var"], 0, 0
    assert not c["cls"].any()
    for s in steps:
        ill, var, sw, _, _ = exact_step(ill, var, c["cls"], s)
        k, margin = k + 1, margin + 2 * s
        inner = (slice(margin, sw.shape[0] - margin), slice(margin, sw.shape[1] - margin))
        assert (sw[inner] == 256).all()
    assert (ill[inner] < 2 ** 24).all()
    var_ok = bool((var[inner] < 2 ** 24).all())
    return ((ill * 2.0 ** (-8 * k)).astype(np.float32), (var * 2.0 ** (-16 * k)).astype(np.float32) if var_ok else None, margin)


# ---- the set-up's inputs ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden(k):
    name, spp = GOLDEN_FRAMES[k]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert int(z["spp"]) == spp
    img = np.ascontiguousarray(z["image"], dtype=np.float32)
    img.setflags(write=False)
    return img, spp


def crop(k, shape):
    img, spp = golden(k)
    ys, xs = SHAPES[shape]
    return np.ascontiguousarray(img[ys, xs]), spp


def setup_inputs():
    """(name, frame, samples, counts): the three golden frames and their crops with their own count, and the 29 x 37 crop of
    the 4-spp frame under a count image of 0, 1, 2, 40 and 2^32 - 1."""
    out = [(f"{GOLDEN_FRAMES[k][0]} {shape}",) + crop(k, shape) + (None,) for k in range(3) for shape in SHAPES]
    frame, _ = crop(1, "29x37")
    counts = np.random.default_rng(5).choice(np.array(COUNT_VALUES, dtype=np.uint32), frame.shape[:2])
    assert set(np.unique(counts).tolist()) == set(COUNT_VALUES)
    out.append(("counts 29x37", frame, 0, counts))
    return out


def guides_of(frame):
    """The two guide images the set-up copies from the frame, without dz: {n.xyz, z} and alb.rgb."""
    return np.concatenate([frame[..., 3:6], frame[..., 9:10]], axis=-1), frame[..., 6:9]


# ---- non-finite frames ------------------------------------------------------------------------------------------------

POISON_AT = {"corner": (0, 0), "left": (13, 0), "top": (0, 17), "inside": (14, 18)}  # (y, x) in the 29 x 37 crop
POISONS = {"nan": (slice(0, 3), np.nan), "inf": (slice(0, 3), np.inf), "nan-var": (slice(10, 11), np.nan)}


def poisoned(where, what):
    """The 29 x 37 crop of the 4-spp golden frame with NaN or +inf planted in the colour, or NaN in channel 10, of one pixel."""
    frame, spp = crop(1, "29x37")
    (y, x), (channels, value) = POISON_AT[where], POISONS[what]
    frame[y, x, channels] = value
    return frame, spp
