"""The fused epilogues of the denoiser's convolution kernel (csrc/pt_denoise.hip: upsample(), epilogue()) restated in NumPy
float32, operation by operation in the kernel's order, so that a layer's output can be demanded bit for bit at sizes where
the bilinear weights are not dyadic.  Written from the kernel's comments and DENOISER.md ("Kernels"), not from its code;
tests/test_denoiser_exact_host.py holds it to the float64 torch upsample so that it cannot share a mistake with the kernel.

What the kernel promises (every operation below is ONE IEEE float32 operation, contraction off, division correctly rounded):

  upsample, align-corners: for output row oy of out_h rows over a map of in_h rows, q = oy (in_h - 1) as an integer,
      h1 = q div (out_h - 1), rem = q mod (out_h - 1), weight h1l = float(rem) / float(out_h - 1), h0l = 1 - h1l;
      an axis of one output row takes h1 = 0, h1l = 0; the "+1" neighbour is row h1 + 1, clamped to the last row.  Columns
      alike.  Value: h0l (w0l p00 + w1l p01) + h1l (w0l p10 + w1l p11).
  lateral:  upsample + relu(acc + bias), one float32 add.
  head:     clip((acc + bias) (float32(0.00316) + albedo), 0, 1), stored as float32 in both modes.
  half mode: the same float32 value, clamped to +-65504, then rounded to fp16 (nearest even); values are read back exactly.

THE BOUND of upsample32 against a float64 upsample (the host test).  With u = 2^-24 and exact weights h0 + h1 = w0 + w1 = 1,
each of the four terms h_a w_b p_ab passes through: its row weight, its column weight, the inner product, the inner sum, the
outer product and the outer sum.  The last four are one rounding each: 4 u relative to the term.  A "+1" weight rem / d is
one rounding: u relative to the term.  The complement 1 - fl(rem / d) is one rounding of its own (u relative) AND inherits the
absolute error of fl(rem / d), u h1, which is not small relative to h0 when h0 is (h0 = 1 / 258 at the largest size here):
u h1 + u h0 = u in absolute terms, i.e. the term's weight h0 replaced by 1.  So, to first order,

    |u32 - u64| <= u [ 4 U(h, w) + U(h~, w) + U(h, w~) ],   h~ = (1, h1), w~ = (1, w1),

where U(a, b) is the interpolation of |up| with row weights a and column weights b (U(h, w) = upsample(|up|)).  Nothing is
fitted: the 4 + 1 + 1 are counted roundings; SLACK = 1 + 2^-20 carries the second-order terms (at most 260 u x 6 u here) and
the float64 reference's own roundings (2^-53 against 2^-24).  A single K for the form K u upsample(|up|) would have to be
4 + max(1, out_h - 1) + max(1, out_w - 1) to be sound by this count (h~ / h0 reaches out_h - 1); the bound above is never
larger than that one and is 6 u upsample(|up|) wherever the complements are not small."""
import numpy as np

KEPS32 = np.float32(0.00316)
HALF_MAX = np.float32(65504.0)
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20


def axis(n_in, n_out):
    """(i0, i1, rem, d) of one axis: source index, its clamped "+1" neighbour, and the weight's integer numerator and
    denominator (rem / d; 0 / 1 on an axis of one output)."""
    o = np.arange(n_out, dtype=np.int64)
    if n_out > 1:
        d = n_out - 1
        q = o * (n_in - 1)
        i0 = q // d
        rem = q - i0 * d
    else:
        d = 1
        i0 = np.zeros(1, np.int64)
        rem = np.zeros(1, np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, rem, d


def weights32(rem, d):
    """(complement, weight) in float32: weight = fl(rem / d), complement = fl(1 - weight)."""
    w1 = rem.astype(np.float32) / np.float32(d)
    return np.float32(1.0) - w1, w1


def interpolate(up, hy, hx, rows, cols):
    """h0 (w0 p00 + w1 p01) + h1 (w0 p10 + w1 p11) in up's dtype, every product and sum rounded to it.  hy = (h0, h1) per
    output row, hx = (w0, w1) per output column, rows = (i0, i1), cols = (j0, j1); up is [in_h][in_w][C]."""
    h0, h1 = (a[:, None, None] for a in hy)
    w0, w1 = (a[None, :, None] for a in hx)
    (r0, r1), (c0, c1) = rows, cols
    p00, p01 = up[r0][:, c0], up[r0][:, c1]
    p10, p11 = up[r1][:, c0], up[r1][:, c1]
    return h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)


def upsample32(up, out_h, out_w):
    """The kernel's upsample of a float32 map [in_h][in_w][C] to [out_h][out_w][C], bit for bit."""
    up = np.ascontiguousarray(up, dtype=np.float32)
    r0, r1, rrem, rd = axis(up.shape[0], out_h)
    c0, c1, crem, cd = axis(up.shape[1], out_w)
    out = interpolate(up, weights32(rrem, rd), weights32(crem, cd), (r0, r1), (c0, c1))
    assert out.dtype == np.float32
    return out


def upsample_bound(up, out_h, out_w):
    """The bound of the module docstring on |upsample32 - float64 upsample|, per element, in float64."""
    a = np.abs(np.asarray(up, dtype=np.float64))
    r0, r1, rrem, rd = axis(a.shape[0], out_h)
    c0, c1, crem, cd = axis(a.shape[1], out_w)
    h1, w1 = rrem / float(rd), crem / float(cd)
    h, w = (1.0 - h1, h1), (1.0 - w1, w1)
    ht, wt = (np.ones_like(h1), h1), (np.ones_like(w1), w1)
    rows, cols = (r0, r1), (c0, c1)
    return U * SLACK * (4.0 * interpolate(a, h, w, rows, cols) + interpolate(a, ht, w, rows, cols) + interpolate(a, h, wt, rows, cols))


def to_stored(v, half):
    """A stored activation as the host reads it back: float32, or in half mode the float32 value clamped to +-65504 and
    rounded to fp16 (nearest even)."""
    v = np.asarray(v, dtype=np.float32)
    if not half:
        return v
    return np.clip(v, -HALF_MAX, HALF_MAX).astype(np.float16).astype(np.float32)


def f32_exact(a):
    """float64 -> float32, asserting that nothing is rounded."""
    a = np.asarray(a, dtype=np.float64)
    b = a.astype(np.float32)
    assert np.array_equal(b.astype(np.float64), a), "not exactly a float32"
    return b


def lateral(acc, bias, up, half=False):
    """EPI_LAT on the accumulation acc [H][W][32] (float32): upsample32(up) + relu(acc + bias), stored."""
    acc, bias = np.asarray(acc, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    v = np.maximum(acc + bias, np.float32(0.0))
    return to_stored(upsample32(up, acc.shape[0], acc.shape[1]) + v, half)


def head(acc, bias, albedo):
    """EPI_RGB on the accumulation acc [H][W][3] (float32): clip((acc + bias) (0.00316f + albedo), 0, 1), float32."""
    acc, bias, albedo = (np.asarray(a, dtype=np.float32) for a in (acc, bias, albedo))
    v = (acc + bias) * (KEPS32 + albedo)
    return np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
