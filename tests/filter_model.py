"""NumPy restatement of the feature-guided filter (include/ptcore.h, pt_filter_*; DENOISER.md, "Feature-guided filter"), for the
tests.  Written from the definition, tap by tap, with a `dtype` parameter: float64 is the yardstick the GPU is held against,
float32 is its twin, whose distance from the yardstick (same measure, same input) scales the GPU's tolerance.

In pieces: setup() is what the kernel's set-up writes (the state {ill, var} and dz), iterate() is one a-trous iteration on a
state (what the lab library's pt_debug_filter_state exports), and filter_model() composes them."""
import numpy as np

EPS32 = np.float32(0.00316)
KERNEL = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0)


def _lum(T, c):
    return T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1] + T(0.0722) * c[..., 2]


def _split(frame, T):
    f = np.asarray(frame, dtype=np.float32).astype(T)  # (float32 -> T is exact)
    return f[..., 0:3], f[..., 3:6], f[..., 6:9], f[..., 9], f[..., 10]


def _neighbours(H, W):
    ys, xs = np.arange(H), np.arange(W)
    return ys, xs, np.clip(ys - 1, 0, H - 1), np.clip(ys + 1, 0, H - 1), np.clip(xs - 1, 0, W - 1), np.clip(xs + 1, 0, W - 1)


def _squared_stop(T, sigma):
    """d2 -> d2 / sigma^2.  The kernel's host code takes 1 / sigma^2 in double and clamps it to the largest finite float, so
    that a sigma whose inverse square overflows is a hard stop (0 stays 0, every difference is refused) and not 0 x inf; here
    likewise: where the double 1 / sigma^2 is beyond `dtype`, the stop multiplies by the largest finite `dtype`.  Every other
    sigma divides by the square formed in `dtype`, as the definition reads."""
    s = float(np.float32(sigma))  # (the options are float32)
    big = float(np.finfo(T).max)
    with np.errstate(over="ignore", under="ignore"):
        if 1.0 / (s * s) > big:
            return lambda d2: d2 * T(big)
        s2 = T(sigma) * T(sigma)
    return lambda d2: d2 / s2


def setup(frame, samples=None, counts=None, dtype=np.float64):
    """frame [H][W][14] float32 -> (ill [H][W][3], var [H][W], dz [H][W], a [H][W][3]) in `dtype`: the demodulated colour, the
    variance of its luminance's mean, the depth gradient and the demodulator EPS + albedo."""
    T = np.dtype(dtype).type
    colour, _, alb, z, cvar = _split(frame, T)
    H, W = z.shape
    with np.errstate(all="ignore"):
        a = T(EPS32) + alb
        ill = colour / a
        n = (np.asarray(counts).astype(T) if counts is not None else np.full((H, W), T(samples), dtype=T))
        la = _lum(T, a)
        li = _lum(T, ill)
        var = np.where(n >= T(2), cvar / np.maximum(n, T(1)) / (la * la), li * li).astype(T)
        ys, xs, yu, yd, xl, xr = _neighbours(H, W)
        dz = T(0.5) * np.maximum(np.abs(z[:, xr] - z[:, xl]), np.abs(z[yd, :] - z[yu, :]))
    return ill, var, dz, a


def iterate(ill, var, frame, dz, step, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0):
    """One iteration at `step` on the state (ill, var) with the guides of `frame` (normal, albedo, depth) and dz -> (ill', var'),
    in the state's dtype.  A tap outside the frame is selected away, not multiplied by 0, and max(g, 0) is fmax: a NaN
    variance does not reach the luminance stop through the blur."""
    T = ill.dtype.type
    _, nrm, alb, z, _ = _split(frame, T)
    H, W = z.shape
    s = int(step)
    ys, xs, yu, yd, xl, xr = _neighbours(H, W)
    stop_n, stop_a = _squared_stop(T, sigma_n), _squared_stop(T, sigma_a)
    with np.errstate(all="ignore"):
        zc = T(1e-3) * np.abs(z) + T(1e-20)
        k3 = (T(0.25), T(0.5), T(0.25))
        g = np.zeros((H, W), dtype=T)
        for r, yy in enumerate((yu, ys, yd)):
            g = g + k3[r] * (k3[0] * var[yy][:, xl] + k3[1] * var[yy][:, xs] + k3[2] * var[yy][:, xr])
        sd = np.sqrt(np.fmax(g, T(0)))
        L = _lum(T, ill)
        den_l = T(sigma_l) * sd + T(0.01) * np.abs(L) + T(1e-4)
        sw = np.zeros((H, W), dtype=T)
        si = np.zeros((H, W, 3), dtype=T)
        sv = np.zeros((H, W), dtype=T)
        for j in range(-2, 3):
            qy = ys + s * j
            vy = (qy >= 0) & (qy < H)
            qyc = np.clip(qy, 0, H - 1)
            for i in range(-2, 3):
                qx = xs + s * i
                vx = (qx >= 0) & (qx < W)
                qxc = np.clip(qx, 0, W - 1)
                valid = vy[:, None] & vx[None, :]
                take = lambda m: m[qyc][:, qxc]
                h = T(KERNEL[i + 2]) * T(KERNEL[j + 2])
                d = T(s) * np.sqrt(T(i * i + j * j))
                dn, da = take(nrm) - nrm, take(alb) - alb
                e = stop_n((dn * dn).sum(-1)) + stop_a((da * da).sum(-1))
                e = e + np.abs(take(z) - z) / (T(sigma_z) * dz * d + zc)
                e = e + np.abs(take(L) - L) / den_l
                w = (h * np.exp(-e)).astype(T)
                sw = sw + np.where(valid, w, T(0))
                si = si + np.where(valid[..., None], w[..., None] * take(ill), T(0))
                sv = sv + np.where(valid, w * w * take(var), T(0))
        return si / sw[..., None], sv / (sw * sw)


def filter_model(frame, samples=None, counts=None, iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0,
                 dtype=np.float64, steps=None):
    """frame [H][W][14] float32 -> the filtered, unclamped radiance [H][W][3] in `dtype`.  samples: the uniform count; counts:
    a [H][W] integer image that replaces it.  steps: the iterations' steps (default 1, 2, 4, ... for `iterations`)."""
    if steps is None:
        steps = [1 << i for i in range(iterations)]
    ill, var, dz, a = setup(frame, samples, counts, dtype)
    for s in steps:
        ill, var = iterate(ill, var, frame, dz, s, sigma_l, sigma_n, sigma_a, sigma_z)
    with np.errstate(all="ignore"):
        out = ill * a
    assert out.dtype == np.dtype(dtype)
    return out


def rel_err(x, ref):
    """The issue's measure: max |x - ref| / (|ref| + 1e-3) over the output, in float64."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(x - ref) / (np.abs(ref) + 1e-3)).max())


def clamped_rms(rgb, ref_rgb):
    """RMS error of the clamped colour (what a display shows) against a reference image."""
    a = np.clip(np.asarray(rgb, dtype=np.float64), 0.0, 1.0)
    b = np.clip(np.asarray(ref_rgb, dtype=np.float64), 0.0, 1.0)
    return float(np.sqrt(((a - b) ** 2).mean()))
