"""The tone-mapping stage (pt_tonemap_*, DENOISER.md "Tone mapping") restated in NumPy float32, operation by operation: the
metered exposure (an integer mean of float bit patterns), the adaptation, the three curves and the two encodes.  Every operation
is a float32 add, multiply, divide or compare, an integer sum or a table lookup, so the kernels are held to it bit for bit.
Also the case builders that tests/test_tonemap_host.py and tests/test_tonemap_gpu.py share."""
import numpy as np

F = np.float32
CLAMP, REINHARD, ACES = 0, 1, 2
SRGB, LINEAR = 0, 1
CURVES = {"clamp": CLAMP, "reinhard": REINHARD, "aces": ACES}
ENCODES = {"srgb": SRGB, "linear": LINEAR}
DEFAULTS = dict(curve=ACES, encode=SRGB, exposure=0.0, key=0.18, white=4.0, adapt=1.0, max_frames=1)
METER_MIN, METER_MAX = 0x35800000, 0x7F7FFFFF  # bits(2^-20) .. bits(FLT_MAX)
X_MAX = F(65504.0)
LOG2_GAP = 0.0861  # max of log2(1 + f) - f on [0, 1): 1 - (1 + ln ln 2) / ln 2 = 0.08607...


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scalar_bits(x):
    """The bit pattern of one float32 as a Python int."""
    return int(np.asarray(x, dtype=np.float32).reshape(()).view(np.uint32))


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def lum(c):
    """(0.2126f x + 0.7152f y) + 0.0722f z, left to right in float32."""
    c = np.asarray(c, dtype=np.float32)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


# ---- encode -----------------------------------------------------------------------------------------------------------

def inverse_oetf(u):
    """sRGB code value u in [0, 1] -> linear light, float64."""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)


def oetf(y):
    """Linear light y in [0, 1] -> sRGB code value, float64."""
    y = np.asarray(y, dtype=np.float64)
    return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.maximum(y, 0.0) ** (1.0 / 2.4) - 0.055)


def srgb_table():
    """T[0 .. 254] = the thresholds of codes 1 .. 255: T[k-1] is the float32 nearest to inverse-OETF((k - 0.5) / 255) formed in
    double.  code(y) = the number of thresholds <= y."""
    k = np.arange(1, 256, dtype=np.float64)
    return inverse_oetf((k - 0.5) / 255.0).astype(np.float32)


def encode(y, mode):
    """float32 y in [0, 1] -> uint8."""
    y = np.asarray(y, dtype=np.float32)
    if mode == SRGB:
        return np.searchsorted(srgb_table(), y, side="right").astype(np.uint8)
    return (y.astype(np.float64) * 255.0).astype(np.uint8)  # (truncation, the display packer's own line)


# ---- meter and adapt --------------------------------------------------------------------------------------------------

def meter(colour):
    """colour [...][3] -> (S, K): the sum of the metered pixels' luminance bit patterns (Python int) and their number."""
    with np.errstate(all="ignore"):
        b = bits(lum(colour)).astype(np.uint64)
    m = (b >= METER_MIN) & (b <= METER_MAX)
    return int(b[m].sum(dtype=np.uint64)), int(m.sum())


def target(S, K, key, prev):
    """The exposure the frame asks for; prev = the exposure before it (None: no history)."""
    if K == 0:
        return F(1.0) if prev is None else F(prev)
    lavg = from_bits(np.uint32(S // K))
    with np.errstate(all="ignore"):
        return F(key) / lavg


def adapt(prev, tgt, rate):
    """prev None (first frame, after a reset) or rate 1: the target's own bits; else two float32 roundings."""
    if prev is None or F(rate) == F(1.0):
        return F(tgt)
    with np.errstate(all="ignore"):
        d = F(tgt) - F(prev)
        return F(prev) + F(rate) * d


# ---- map --------------------------------------------------------------------------------------------------------------

def curve_map(colour, e, curve, white=4.0):
    """colour [...][3] float32, exposure e -> y [...][3] float32 in [0, 1], never NaN."""
    c = np.asarray(colour, dtype=np.float32)
    with np.errstate(all="ignore"):
        x = c * F(e)
        x = np.where(x > 0, x, F(0.0))
        x = np.where(x < X_MAX, x, X_MAX)
        if curve == CLAMP:
            y = x
        elif curve == REINHARD:
            lx = lum(x)
            w2 = F(white) * F(white)
            s = (F(1.0) + lx / w2) / (F(1.0) + lx)
            y = x * s[..., None]
        elif curve == ACES:
            y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        else:
            raise ValueError(curve)
        y = np.where(y < 1, y, F(1.0))
    assert y.dtype == np.float32
    return y


def map_encode(colour, e, curve=ACES, enc=SRGB, white=4.0):
    """-> uint8 [...][4]: r, g, b, 255."""
    y = curve_map(colour, e, curve, white)
    out = np.empty(y.shape[:-1] + (4,), np.uint8)
    out[..., :3] = encode(y, enc)
    out[..., 3] = 255
    return out


def tonemap_sequence(frames, curve=ACES, enc=SRGB, exposure=0.0, key=0.18, white=4.0, rate=1.0, prev=None):
    """frames: an iterable of [H][W][>= 3] float32 images in order through one session that holds exposure `prev` (None: fresh or
    reset).  -> (list of uint8 [H][W][4], list of the float32 exposure after each frame)."""
    outs, exps = [], []
    for f in frames:
        c = np.asarray(f, dtype=np.float32)[..., :3]
        if exposure != 0.0:
            e = F(exposure)
        else:
            S, K = meter(c)
            e = adapt(prev, target(S, K, key, prev), rate)
            prev = e
        outs.append(map_encode(c, e, curve, enc, white))
        exps.append(F(e))
    return outs, exps


# ---- case builders ----------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (64, 3), (3, 64), (37, 29), (64, 64), (300, 70)]  # (width, height)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 1e-45, 1e-39, 65504.0, 3.0e38, 2.0 ** -20, 1.0], np.float32)


def random_frame(width, height, stride, seed):
    """Radiance log-uniform over 2^-24 .. 2^12 in the colour channels, other channels noise; NaN, +-inf, negatives, zeros and
    denormals planted into about an eighth of the pixels (every special value lands in each channel when the frame is large
    enough; a 1 x 1 frame keeps its random pixel so that the meter has something to count for odd seeds)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((height, width, stride)).astype(np.float32)
    f[..., :3] = np.exp2(rng.uniform(-24.0, 12.0, (height, width, 3))).astype(np.float32)
    n = height * width
    flat = f.reshape(n, stride)
    if n > 1 or seed % 2 == 0:
        k = max(1, n // 8)
        where = rng.choice(n, size=k, replace=False)
        flat[where, rng.integers(0, 3, k)] = SPECIALS[np.arange(k) % len(SPECIALS)]
    return f


def threshold_frame(stride=3):
    """[6][255][stride]: row 2 c holds T[k] in channel c and row 2 c + 1 nextafter(T[k], 0), the other channels 0.25."""
    T = srgb_table()
    f = np.full((6, 255, stride), 0.25, np.float32)
    for c in range(3):
        f[2 * c, :, c] = T
        f[2 * c + 1, :, c] = np.nextafter(T, F(0.0))
    return f


def stepped_frames(width, height, stride, n=6, seed=5):
    """n frames of one random image, frame k brighter than frame k-1 by x 8 (exact in float32)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((height, width, stride)).astype(np.float32)
    base[..., :3] = np.exp2(rng.uniform(-12.0, -2.0, (height, width, 3))).astype(np.float32)
    out = np.repeat(base[None], n, axis=0)
    for k in range(n):
        out[k, ..., :3] *= F(8.0 ** k)
    return out


def lognormal_image(width, height, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(-1.0, sigma, (height, width, 3))).astype(np.float32)
