"""The comparison stage (pt_compare_*, DENOISER.md "Frame comparison") restated in NumPy float32, operation by operation: the
sanitised values, the clamped squared error m, the capped relative squared error r, the SSIM s of the display luminances with
an 11 x 11 Gaussian window and replicated edges, and the three integer sums.  Every operation is a float32 add, multiply, divide
or compare or an integer sum, so the kernels are held to it bit for bit.  `twin` is the same definition in float64 with true
means (no float32 rounding, no quantisation): the reference the float32 definition itself is judged against.  Also the case
builders that tests/test_compare_host.py and tests/test_compare_gpu.py share."""
import math

import numpy as np

F = np.float32
X_MAX = F(65504.0)
R_CAP, R_EPS = F(1024.0), F(0.01)
C1, C2 = F(0.01) * F(0.01), F(0.03) * F(0.03)
TAPS, RADIUS, SIGMA = 11, 5, 1.5
QM, QR, QS = 2.0 ** 34, 2.0 ** 24, 2.0 ** 32
FIELDS = ("sum_mse", "sum_relmse", "sum_ssim", "pixels", "saturated", "nonfinite", "mse", "rms", "psnr", "relmse", "ssim")
SIZES = [(1, 1), (16, 16), (17, 15), (37, 29), (300, 70)]  # (width, height): one pixel, one tile, ragged, three tiles + edges, many


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def double_bits(x):
    return int(np.asarray(x, dtype=np.float64).reshape(()).view(np.uint64))


def weights64():
    """exp(-(k - 5)^2 / (2 sigma^2)) in double, divided by their sum (added from k = 0 up).  math.exp, not np.exp: the library
    calls the C library's exp."""
    g = [math.exp(-((k - RADIUS) * (k - RADIUS)) / (2.0 * SIGMA * SIGMA)) for k in range(TAPS)]
    total = 0.0
    for v in g:
        total += v
    return np.array([v / total for v in g], dtype=np.float64)


def weights():
    """The eleven float32 weights of pt_compare_ssim_weights."""
    return weights64().astype(np.float32)


def lum(c):
    """(0.2126f x + 0.7152f y) + 0.0722f z, left to right in float32."""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def sanitise(c):
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(c > 0, c, F(0.0))  # (NaN becomes 0)
        return np.where(x < X_MAX, x, X_MAX)


def blur(q, w):
    """One separable pass pair on q [H][W]: along the row, then along the column; taps from the lowest offset to the highest, one
    add per tap; coordinates clamp."""
    def one(q, axis):
        n = q.shape[axis]
        idx = np.arange(n)
        acc = w[0] * np.take(q, np.clip(idx - RADIUS, 0, n - 1), axis=axis)
        for k in range(1, TAPS):
            acc = acc + w[k] * np.take(q, np.clip(idx + (k - RADIUS), 0, n - 1), axis=axis)
        return acc
    return one(one(q, 1), 0)


def derive(sum_m, sum_r, sum_s, pixels):
    """Step 6 of the definition, in Python doubles (math.sqrt and math.log10: the C library's)."""
    mse = float(sum_m) / QM / (3.0 * pixels)
    return dict(mse=mse, rms=math.sqrt(mse), psnr=-10.0 * math.log10(mse) if mse > 0.0 else math.inf,
                relmse=float(sum_r) / QR / (3.0 * pixels), ssim=float(sum_s) / QS / pixels)


def compare(img, ref):
    """img, ref [H][W][>= 3] float32 -> dict: the maps m, r, s [H][W] float32 and every field of pt_compare_values."""
    ca, cb = np.asarray(img, dtype=np.float32)[..., :3], np.asarray(ref, dtype=np.float32)[..., :3]
    h, w = ca.shape[:2]
    a, b = sanitise(ca), sanitise(cb)
    da, db = np.where(a < 1, a, F(1.0)), np.where(b < 1, b, F(1.0))
    d = da - db
    t = d * d
    m = (t[..., 0] + t[..., 1]) + t[..., 2]
    d = a - b
    t = (d * d) / (b * b + R_EPS)
    hit = ~(t < R_CAP)
    t = np.where(hit, R_CAP, t)
    r = (t[..., 0] + t[..., 1]) + t[..., 2]
    la, lb = lum(da), lum(db)
    wt = weights()
    ua, ub, eaa, ebb, eab = (blur(q, wt) for q in (la, lb, la * la, lb * lb, la * lb))
    mab, maa, mbb = ua * ub, ua * ua, ub * ub
    va, vb, cab = eaa - maa, ebb - mbb, eab - mab
    s = ((F(2.0) * mab + C1) * (F(2.0) * cab + C2)) / (((maa + mbb) + C1) * ((va + vb) + C2))
    for x in (m, r, s):
        assert x.dtype == np.float32
    qm = np.floor(m.astype(np.float64) * QM).astype(np.uint64)
    qr = np.floor(r.astype(np.float64) * QR).astype(np.uint64)
    qs = np.floor(s.astype(np.float64) * QS).astype(np.int64)
    out = dict(m=m, r=r, s=s, sum_mse=int(qm.sum(dtype=np.uint64)), sum_relmse=int(qr.sum(dtype=np.uint64)), sum_ssim=int(qs.sum(dtype=np.int64)),
               pixels=h * w, saturated=int(hit.sum()), nonfinite=int((~np.isfinite(ca).all(axis=-1) | ~np.isfinite(cb).all(axis=-1)).sum()))
    out.update(derive(out["sum_mse"], out["sum_relmse"], out["sum_ssim"], h * w))
    return out


def stack(res):
    """The map [H][W][3] = (m, r, s) the device writes."""
    return np.stack([res["m"], res["r"], res["s"]], axis=-1)


def twin(img, ref):
    """The same definition in float64: true means, double weights, no quantisation.  -> dict m, r, s [H][W] float64 and the frame
    values mse, relmse, ssim."""
    ca, cb = np.asarray(img, dtype=np.float32)[..., :3].astype(np.float64), np.asarray(ref, dtype=np.float32)[..., :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        a, b = (np.minimum(np.where(c > 0, c, 0.0), 65504.0) for c in (ca, cb))
    da, db = np.minimum(a, 1.0), np.minimum(b, 1.0)
    m = ((da - db) ** 2).sum(axis=-1)
    r = np.minimum((a - b) ** 2 / (b * b + 0.01), 1024.0).sum(axis=-1)
    k = np.array([0.2126, 0.7152, 0.0722])
    la, lb = da @ k, db @ k
    wt = weights64()
    ua, ub, eaa, ebb, eab = (blur(q, wt) for q in (la, lb, la * la, lb * lb, la * lb))
    va, vb, cab = eaa - ua * ua, ebb - ub * ub, eab - ua * ub
    s = ((2 * ua * ub + 1e-4) * (2 * cab + 9e-4)) / ((ua * ua + ub * ub + 1e-4) * (va + vb + 9e-4))
    return dict(m=m, r=r, s=s, mse=m.mean() / 3.0, relmse=r.mean() / 3.0, ssim=s.mean())


# ---- case builders ----------------------------------------------------------------------------------------------------

SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.5, 0.0, 1.0, 65504.0, 1e5, 1e-45, -0.0], np.float32)


def hdr_pair(width, height, seed, img_stride=3, ref_stride=3):
    """A lognormal image (tonemap_model.lognormal_image) and a reference that is the same picture with multiplicative noise, in
    frames of the given pixel strides (the other channels noise); NaN, +-inf, negatives, exactly 1.0, 65504 and a value above it
    planted into about an eighth of the pixels of each (a 1 x 1 frame gets one special in the image only)."""
    import tonemap_model as tm

    rng = np.random.default_rng(seed)
    base = tm.lognormal_image(width, height, seed)
    noisy = (base * np.exp(rng.normal(0.0, 0.5, base.shape))).astype(np.float32)
    out = []
    for colour, stride, salt in ((noisy, img_stride, 1), (base, ref_stride, 2)):
        f = rng.standard_normal((height, width, stride)).astype(np.float32)
        f[..., :3] = colour
        n = height * width
        flat = f.reshape(n, stride)
        if n > 1 or salt == 1:
            k = max(1, n // 8)
            where = rng.choice(n, size=k, replace=False)
            flat[where, rng.integers(0, 3, k)] = SPECIALS[(np.arange(k) + salt) % len(SPECIALS)]
        out.append(f)
    return out[0], out[1]
