"""NumPy restatement of the feature-guided filter (include/ptcore.h, pt_filter_*; DENOISER.md, "Feature-guided filter"), for the
tests.  Written from the definition, tap by tap, with a `dtype` parameter: float64 is the yardstick the GPU is held against,
float32 is its twin, whose distance from the yardstick (same measure, same input) scales the GPU's tolerance."""
import numpy as np

EPS32 = np.float32(0.00316)
KERNEL = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0)


def _lum(T, c):
    return T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1] + T(0.0722) * c[..., 2]


def filter_model(frame, samples=None, counts=None, iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0,
                 dtype=np.float64, steps=None):
    """frame [H][W][14] float32 -> the filtered, unclamped radiance [H][W][3] in `dtype`.  samples: the uniform count; counts:
    a [H][W] integer image that replaces it.  steps: the iterations' steps (default 1, 2, 4, ... for `iterations`)."""
    T = np.dtype(dtype).type
    f = np.asarray(frame, dtype=np.float32).astype(T)  # (float32 -> T is exact)
    H, W = f.shape[:2]
    if steps is None:
        steps = [1 << i for i in range(iterations)]
    with np.errstate(over="ignore", under="ignore"):
        colour, nrm, alb, z, cvar = f[..., 0:3], f[..., 3:6], f[..., 6:9], f[..., 9], f[..., 10]
        a = T(EPS32) + alb
        ill = colour / a
        n = (np.asarray(counts).astype(T) if counts is not None else np.full((H, W), T(samples), dtype=T))
        la = _lum(T, a)
        li = _lum(T, ill)
        var = np.where(n >= T(2), cvar / np.maximum(n, T(1)) / (la * la), li * li).astype(T)
        ys, xs = np.arange(H), np.arange(W)
        yu, yd, xl, xr = np.clip(ys - 1, 0, H - 1), np.clip(ys + 1, 0, H - 1), np.clip(xs - 1, 0, W - 1), np.clip(xs + 1, 0, W - 1)
        dz = T(0.5) * np.maximum(np.abs(z[:, xr] - z[:, xl]), np.abs(z[yd, :] - z[yu, :]))
        sn2, sa2 = T(sigma_n) * T(sigma_n), T(sigma_a) * T(sigma_a)
        zc = T(1e-3) * np.abs(z) + T(1e-20)
        for s in steps:
            k3 = (T(0.25), T(0.5), T(0.25))
            g = np.zeros((H, W), dtype=T)
            for r, yy in enumerate((yu, ys, yd)):
                g = g + k3[r] * (k3[0] * var[yy][:, xl] + k3[1] * var[yy][:, xs] + k3[2] * var[yy][:, xr])
            sd = np.sqrt(np.maximum(g, T(0)))
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
                    e = (dn * dn).sum(-1) / sn2 + (da * da).sum(-1) / sa2
                    e = e + np.abs(take(z) - z) / (T(sigma_z) * dz * d + zc)
                    e = e + np.abs(take(L) - L) / den_l
                    w = np.where(valid, h * np.exp(-e), T(0)).astype(T)
                    sw = sw + w
                    si = si + w[..., None] * take(ill)
                    sv = sv + w * w * take(var)
            ill = si / sw[..., None]
            var = sv / (sw * sw)
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
