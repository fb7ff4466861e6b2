"""NumPy restatement of the feature filter's spatial variance estimate (include/ptcore.h, pt_filter_set_spatial; DENOISER.md,
"Spatial variance estimate"), for the tests.  Written from the definition with a `dtype` parameter like tests/filter_model.py,
which it imports and leaves alone: float64 is the yardstick, float32 its twin.

After the set-up, every pixel p whose integer count n_p is below `below` gets var_p <- fmax(var_p, v), v the weighted spread of
the luminances L = lum(ill) in the (2R+1)^2 window around p, weighted by the filter's own normal, albedo and depth stops (no
luminance stop).  Two passes, centred; the window is walked row by row, and a tap outside the frame is selected away.  Both
passes work on L_q - L_p, the luminance relative to the pixel's own: mathematically the same v, but a window of equal luminances
then gives exactly 0 in any precision instead of the rounding of its mean, squared."""
import numpy as np

import filter_model as fm

ALL = 0xFFFFFFFF  # PT_FILTER_SPATIAL_ALL: every pixel


def counts_of(shape, samples=None, counts=None):
    """The integer count image the rule `n_p < below` reads: the count image if one is given, else the uniform `samples`."""
    if counts is not None:
        return np.asarray(counts).astype(np.uint64)
    return np.full(shape, int(samples), dtype=np.uint64)


def estimate(ill, frame, dz, radius=2, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0):
    """(v [H][W], sum of the weights [H][W], sum of their squares [H][W]) in ill's dtype: the estimate of every pixel, whatever
    its count."""
    T = ill.dtype.type
    _, nrm, alb, z, _ = fm._split(frame, T)
    H, W = z.shape
    R = int(radius)
    ys, xs = np.arange(H), np.arange(W)
    stop_n, stop_a = fm._squared_stop(T, sigma_n), fm._squared_stop(T, sigma_a)
    with np.errstate(all="ignore"):
        L = fm._lum(T, ill)
        zc = T(1e-3) * np.abs(z) + T(1e-20)
        taps = []
        sw, sl, sw2 = np.zeros((H, W), dtype=T), np.zeros((H, W), dtype=T), np.zeros((H, W), dtype=T)
        for j in range(-R, R + 1):
            qy = ys + j
            vy = (qy >= 0) & (qy < H)
            qyc = np.clip(qy, 0, H - 1)
            for i in range(-R, R + 1):
                qx = xs + i
                vx = (qx >= 0) & (qx < W)
                qxc = np.clip(qx, 0, W - 1)
                valid = vy[:, None] & vx[None, :]
                take = lambda m: m[qyc][:, qxc]
                if i == 0 and j == 0:
                    w = np.ones((H, W), dtype=T)
                else:
                    d = np.sqrt(T(i * i + j * j))
                    dn, da = take(nrm) - nrm, take(alb) - alb
                    e = stop_n((dn * dn).sum(-1)) + stop_a((da * da).sum(-1))
                    e = e + np.abs(take(z) - z) / (T(sigma_z) * dz * d + zc)
                    w = np.exp(-e).astype(T)
                Lq = take(L) - L  # the moments are taken of L_q - L_p: the same m - L_p and v, and exactly 0 on a flat window
                taps.append((valid, w, Lq))
                sw = np.where(valid, sw + w, sw)
                sl = np.where(valid, sl + w * Lq, sl)
                sw2 = np.where(valid, sw2 + w * w, sw2)
        m = sl / sw
        sv = np.zeros((H, W), dtype=T)
        for valid, w, Lq in taps:
            dl = Lq - m
            sv = np.where(valid, sv + w * (dl * dl), sv)
        v = sv / sw
    assert v.dtype == np.dtype(T)
    return v, sw, sw2


def spatial_var(ill, var, frame, dz, below, radius=2, samples=None, counts=None, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0):
    """The variance image after the estimate: fmax(var, v) where the pixel's count is below `below`, var itself (bit for bit)
    elsewhere.  fmax: a NaN v leaves var as it was."""
    n = counts_of(var.shape, samples, counts)
    low = n < np.uint64(int(below))
    if not low.any():
        return var
    v = estimate(ill, frame, dz, radius, sigma_n, sigma_a, sigma_z)[0]
    return np.where(low, np.fmax(var, v), var).astype(var.dtype)


def setup(frame, samples=None, counts=None, below=0, radius=2, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0, dtype=np.float64):
    """fm.setup() followed by the estimate: (ill, var, dz, a)."""
    ill, var, dz, a = fm.setup(frame, samples, counts, dtype)
    var = spatial_var(ill, var, frame, dz, below, radius, samples, counts, sigma_n, sigma_a, sigma_z)
    return ill, var, dz, a


def filter_model(frame, samples=None, counts=None, below=0, radius=2, iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1,
                 sigma_z=1.0, dtype=np.float64, steps=None):
    """fm.filter_model() with the estimate between the set-up and the first iteration.  below = 0 is fm.filter_model()."""
    if steps is None:
        steps = [1 << i for i in range(iterations)]
    ill, var, dz, a = setup(frame, samples, counts, below, radius, sigma_n, sigma_a, sigma_z, dtype)
    for s in steps:
        ill, var = fm.iterate(ill, var, frame, dz, s, sigma_l, sigma_n, sigma_a, sigma_z)
    with np.errstate(all="ignore"):
        out = ill * a
    assert out.dtype == np.dtype(dtype)
    return out
