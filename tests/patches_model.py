"""The training-patch stage (pt_patches_*, DENOISER.md "Training patches") restated in NumPy float32, operation by operation: the
divisors of a frame, the pre-processed pixel, the score of a patch as eight integer sums (Python integers stand in for the
128-bit arithmetic of pt_patches_result) and the gathered tensors.  Every operation is a float32 divide or compare, a floor of a
double product or an integer sum, so the kernels are held to it bit for bit.  `twin` is the reference's measure on the same
values: np.var in float64 on the pre-processed float32 patch (load_data.py: get_score).  Also the case builders that
tests/test_patches_host.py and tests/test_patches_gpu.py share."""
import numpy as np

F = np.float32
EPS = F(0.00316)
X_MAX = F(65504.0)
Q = 2.0 ** 20
SUMS = ("colour_s1", "colour_a", "colour_b", "colour_c", "normal_s1", "normal_a", "normal_b", "normal_c")
DOUBLES = ("var_colour", "var_normal", "score")
FIELDS = SUMS + ("values",) + DOUBLES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def double_bits(x):
    return int(np.asarray(x, dtype=np.float64).reshape(()).view(np.uint64))


# ---- steps 1 and 2 ----------------------------------------------------------------------------------------------------

def divisors(frame):
    """Step 1: (float)(0.00316 + (double)m_k), m_k the maximum of channel k in 9 .. 13 by fmaxf from -inf (NaNs are ignored)."""
    f = np.asarray(frame, dtype=np.float32)
    out = np.empty(5, np.float32)
    for k in range(5):
        m = np.fmax.reduce(f[..., 9 + k].ravel(), initial=F(-np.inf))
        out[k] = F(0.00316 + float(m))
    return out


def preprocess(frame):
    """Step 2 on the whole frame [H][W][14] -> float32 [H][W][14]."""
    f = np.array(frame, dtype=np.float32, copy=True)
    div = divisors(f)
    with np.errstate(all="ignore"):
        f[..., 0:3] = f[..., 0:3] / (EPS + f[..., 6:9])
        for k in range(5):
            f[..., 9 + k] = f[..., 9 + k] / div[k]
    assert f.dtype == np.float32
    return f


# ---- step 3 -----------------------------------------------------------------------------------------------------------

def sanitise_colour(x):
    with np.errstate(invalid="ignore"):
        v = np.where(x > 0, x, F(0.0))  # (NaN becomes 0)
        return np.where(v < X_MAX, v, X_MAX).astype(np.float32)


def sanitise_normal(x):
    with np.errstate(invalid="ignore"):
        v = np.where(x == x, x, F(0.0))
        v = np.where(v < X_MAX, v, X_MAX)
        return np.where(v > -X_MAX, v, -X_MAX).astype(np.float32)


def population_sums(v):
    """The sanitised float32 values of one population -> (S1, A, B, C) as Python integers."""
    q = np.floor(np.asarray(v, dtype=np.float32).astype(np.float64) * Q).astype(np.int64).ravel()
    a = np.abs(q).astype(np.uint64)
    ah, al = a >> np.uint64(18), a & np.uint64((1 << 18) - 1)
    return (int(q.sum(dtype=np.int64)), int((ah * ah).sum(dtype=np.uint64)), int((ah * al).sum(dtype=np.uint64)),
            int((al * al).sum(dtype=np.uint64)))


def variance(s1, a, b, c, n):
    """pt_patches_result's arithmetic: integers until one conversion (float(int) rounds to nearest even), then two divisions."""
    s2 = (a << 36) + (b << 19) + c
    num = n * s2 - s1 * s1
    assert num >= 0
    return (float(num) / float(n * n)) / 2.0 ** 40


def derive(sums, n):
    """The eight sums and N -> every field of pt_patches_values."""
    out = dict(zip(SUMS, sums))
    out["values"] = n
    out["var_colour"] = variance(*sums[0:4], n)
    out["var_normal"] = variance(*sums[4:8], n)
    out["score"] = out["var_colour"] + out["var_normal"]
    return out


def score_values(colour, normal):
    """Step 3 on the two populations' (pre-processed, unsanitised) values."""
    colour, normal = np.asarray(colour, dtype=np.float32), np.asarray(normal, dtype=np.float32)
    assert colour.size == normal.size
    return derive(population_sums(sanitise_colour(colour)) + population_sums(sanitise_normal(normal)), colour.size)


def score(pre, corner, p):
    """Step 3 for the patch with corner (x, y) of the pre-processed frame `pre`."""
    x, y = corner
    patch = pre[y:y + p, x:x + p]
    assert patch.shape[:2] == (p, p)
    return score_values(patch[..., 0:3], patch[..., 3:6])


def scores(frame, corners, p):
    pre = preprocess(frame)
    return [score(pre, c, p) for c in corners]


def twin(pre, corner, p):
    """The reference's get_score on the same float32 values: np.var in float64 of the colour plus that of the normal."""
    x, y = corner
    patch = pre[y:y + p, x:x + p].astype(np.float64)
    return float(np.var(patch[..., 0:3])), float(np.var(patch[..., 3:6]))


# ---- step 4 -----------------------------------------------------------------------------------------------------------

def gather(frame, gt, corners, p):
    """-> (inputs [n][14][P][P], targets [n][3][P][P]) float32; [k][c][j][i] is pixel (y_k + j, x_k + i)."""
    pre = preprocess(frame)
    g = np.asarray(gt, dtype=np.float32)[..., :3]
    with np.errstate(invalid="ignore"):
        t = np.where(g > 0, g, F(0.0))  # (NaN becomes 0)
        t = np.where(t < 1, t, F(1.0)).astype(np.float32)
    inputs = np.stack([pre[y:y + p, x:x + p].transpose(2, 0, 1) for x, y in corners])
    targets = np.stack([t[y:y + p, x:x + p].transpose(2, 0, 1) for x, y in corners])
    assert inputs.shape == (len(corners), 14, p, p) and targets.shape == (len(corners), 3, p, p)
    return np.ascontiguousarray(inputs), np.ascontiguousarray(targets)


# ---- case builders ------------------------------------------------------------------------------------------------------

SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.5, 0.0, 1.0, 65504.0, 1e5, 1e-45, -0.0], np.float32)

# (width, height, patch): ragged against every lane count twice, the patch as high as the frame, one pixel, the patch is the
# frame, a patch of several score workgroups whose rows are half a staging run
SIZES = [(37, 29, 5), (37, 29, 8), (64, 48, 48), (37, 29, 1), (16, 16, 16), (96, 80, 64)]


def frame_pair(width, height, seed, gt_stride=3, specials=True, nan_features=False):
    """A train frame [H][W][14] and a target image [H][W][gt_stride]: lognormal HDR colour, normals in [-1, 1], albedo in [0, 1]
    with exact zeros, depth and variances (channels 9-13) finite and >= 0 as the renderer writes them; the target is the same
    picture with less noise, its other channels noise.  specials: NaN, +-inf, negatives, exactly 1.0, 65504 and more planted in
    about an eighth of the pixels of colour, normal and albedo and of the target's colour.  nan_features: a NaN in each of
    channels 9-13 too (what fmaxf must ignore)."""
    rng = np.random.default_rng(seed)
    n = height * width
    base = np.exp(rng.normal(-1.0, 1.5, (height, width, 3)))
    f = np.empty((height, width, 14), np.float32)
    f[..., 0:3] = base * np.exp(rng.normal(0.0, 0.5, base.shape))
    f[..., 3:6] = rng.uniform(-1.0, 1.0, (height, width, 3))
    f[..., 6:9] = rng.uniform(0.0, 1.0, (height, width, 3))
    f[..., 6:9][rng.random((height, width, 3)) < 0.1] = 0.0
    f[..., 9] = rng.uniform(0.0, 300.0, (height, width))
    f[..., 10:14] = np.exp(rng.normal(-2.0, 1.0, (height, width, 4)))
    g = rng.standard_normal((height, width, gt_stride)).astype(np.float32)
    g[..., :3] = base * np.exp(rng.normal(0.0, 0.05, base.shape))
    if specials:
        k = max(1, n // 8)
        for flat, channels, salt in ((f.reshape(n, 14), 9, 1), (g.reshape(n, gt_stride), 3, 2)):
            where = rng.choice(n, size=k, replace=False)
            flat[where, rng.integers(0, channels, k)] = SPECIALS[(np.arange(k) + salt) % len(SPECIALS)]
    if nan_features:
        flat = f.reshape(n, 14)
        for c in range(9, 14):
            flat[rng.integers(0, n), c] = np.nan
    return f, g


def corner_list(width, height, p):
    """(0, 0), (W - P, H - P), the other two extremes, odd offsets that misalign every 16-byte store, a duplicate and heavily
    overlapping neighbours, each clipped into the frame: 10 corners."""
    mx, my = width - p, height - p
    raw = [(0, 0), (mx, my), (mx, 0), (0, my), (1, 1), (3, 2), (1, 1), (2, 1), (mx - 1, my - 3), (mx // 2 + 1, my // 2)]
    return [(min(max(x, 0), mx), min(max(y, 0), my)) for x, y in raw]
