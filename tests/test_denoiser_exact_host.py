"""tests/denoise_exact_model.py, the float32 restatement of the denoiser's lateral and head epilogues that the exact GPU test
(tests/test_denoiser_exact_gpu.py) compares bits with, held to float64 on the CPU: the restatement mirrors the kernel, so
without this it could share a mistake with it.  The bounds count roundings (the model's docstring); none is fitted."""
import numpy as np
import pytest
import torch

import denoise_exact_model as EM
import denoise_restatement as R

PAIRS = [((1, 1), (2, 3)), ((1, 1), (1, 2)), ((1, 2), (4, 5)), ((2, 3), (8, 10)), ((8, 10), (29, 37)), ((64, 65), (253, 259))]
SIZES = [p for a, b in PAIRS for p in ((a, b), (a[::-1], b[::-1]))]  # both orientations, (rows, columns)


def upsample64(up, out_h, out_w):
    """R.upsample (torch, align-corners, float64) of an [h][w][C] map."""
    t = torch.from_numpy(np.ascontiguousarray(up, dtype=np.float64)).permute(2, 0, 1).unsqueeze(0)
    return R.upsample(t, (out_h, out_w))[0].permute(1, 2, 0).numpy()


def _map(rs, shape):
    """Random float32 values over a few decades and both signs, so that neighbours of very different size meet."""
    return (rs.normal(0.0, 1.0, shape) * 10.0 ** rs.uniform(-2.0, 2.0, shape)).astype(np.float32)


@pytest.mark.parametrize("src,dst", SIZES, ids=[f"{a[0]}x{a[1]}-to-{b[0]}x{b[1]}" for a, b in SIZES])
def test_upsample32_is_the_float64_upsample_within_its_roundings(src, dst, capsys):
    """|upsample32 - R.upsample| <= 2^-24 [4 U(h, w) + U(h~, w) + U(h, w~)] of |up| (denoise_exact_model: four roundings of
    the interpolation, one of each weight, the complement's inherited absolute error), and U(h, w) itself is the float64
    upsample of |up| (the bound is built on the right indices and weights).  Prints the worst error in units of
    2^-24 upsample(|up|)."""
    rs = np.random.default_rng(src[0] * 1000 + src[1] * 10 + dst[0])
    up = _map(rs, src + (32,))
    u32 = EM.upsample32(up, *dst)
    u64 = upsample64(up, *dst)
    a64 = upsample64(np.abs(up), *dst)
    assert u32.shape == u64.shape == dst + (32,) and u32.dtype == np.float32
    bound = EM.upsample_bound(up, *dst)
    assert np.all(bound >= 6.0 * EM.U * a64 * (1.0 - 1e-9)) and np.all(bound <= (4.0 + max(1, dst[0] - 1) + max(1, dst[1] - 1)) * EM.U * EM.SLACK * a64 * (1.0 + 1e-9) + 1e-300)
    err = np.abs(u32.astype(np.float64) - u64)
    with capsys.disabled():
        print(f"\n{src} -> {dst}: worst |u32 - u64| = {float(np.max(err / np.maximum(EM.U * a64, 1e-300))):.2f} x 2^-24 upsample(|up|)")
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, f"{len(bad)} outside the bound, first {bad[:3].tolist()}: {u32[tuple(bad[0])]} vs {u64[tuple(bad[0])]}"
    # the corners of an align-corners upsample are the corners of the map, exactly
    for (oy, iy) in ((0, 0), (dst[0] - 1, src[0] - 1)):
        for (ox, ix) in ((0, 0), (dst[1] - 1, src[1] - 1)):
            assert np.array_equal(u32[oy, ox], up[iy, ix])


def test_lateral_epilogue_within_its_roundings():
    """lateral() = upsample(up) + relu(acc + bias) in float64 within: the upsample's bound, one rounding of acc + bias and one
    of the final add.  Half mode: one more rounding, to fp16."""
    rs = np.random.default_rng(21)
    acc = _map(rs, (29, 37, 32))
    bias = rs.normal(0.0, 1.0, 32).astype(np.float32)
    up = _map(rs, (8, 10, 32))
    v64 = np.maximum(acc.astype(np.float64) + bias.astype(np.float64), 0.0)
    u64 = upsample64(up, 29, 37)
    ref = u64 + v64
    bound = EM.upsample_bound(up, 29, 37) + EM.U * EM.SLACK * (v64 + (upsample64(np.abs(up), 29, 37) + v64))
    got = EM.lateral(acc, bias, up)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - ref) <= bound)
    assert (v64 > 0).any() and (v64 == 0).any()
    half = EM.lateral(acc, bias, up, half=True)
    assert np.array_equal(half, half.astype(np.float16).astype(np.float32)) and np.abs(half).max() <= 65504.0
    clipped = np.clip(ref, -65504.0, 65504.0)  # fp16: half an ulp is at most 2^-11 of a normal value, 2^-25 of a subnormal one
    assert np.all(np.abs(half.astype(np.float64) - clipped) <= bound + 2.0 ** -11 * (np.abs(clipped) + bound) + 2.0 ** -25)
    big = EM.lateral(np.full((1, 1, 32), 1e6, np.float32), bias, np.zeros((1, 1, 32), np.float32), half=True)
    assert np.all(big == np.float32(65504.0))  # saturates, never an infinity


def test_head_epilogue_within_its_roundings():
    """head() = clip((acc + bias) (0.00316 + albedo), 0, 1) in float64 within four roundings of the unclipped product: the
    float32 constant, the two sums and the product (the clip does not increase a difference)."""
    rs = np.random.default_rng(22)
    acc = rs.normal(0.0, 3.0, (29, 37, 3)).astype(np.float32)
    bias = rs.normal(0.0, 1.0, 3).astype(np.float32)
    alb = rs.uniform(0.0, 1.0, (29, 37, 3)).astype(np.float32)
    raw = (acc.astype(np.float64) + bias.astype(np.float64)) * (R.KEPS + alb.astype(np.float64))
    ref = np.clip(raw, 0.0, 1.0)
    got = EM.head(acc, bias, alb)
    assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 4.0 * EM.U * EM.SLACK * np.abs(raw))
    inside = float(((ref > 0) & (ref < 1)).mean())
    assert 0.2 < inside < 0.8 and (ref == 0).any() and (ref == 1).any(), inside
