"""Synthetic sequences for the temporal accumulator (DENOISER.md, "Temporal accumulation") on which every float32 operation of
the definition is exact, with the output they must give worked out from plane geometry in float64 -- without P, without
tests/temporal_model.py and without a rounding.  NumPy and the standard library only; shared by test_temporal_exact_host.py (the
model against these expectations) and test_temporal_exact_gpu.py (the kernel against them and against the model).

The camera: B0 = (-0.5, -0.25, -1), B1 - B0 = (2, 0, 0), B2 - B0 = (0, 1, 0), eye (50, 52, 295.5); det [B0 | B1-B0 | B2-B0] = -2,
so P is dyadic.  The renderer's primary ray of pixel (row r, column c) is d = B0 + (c / H) (B1 - B0) + (1 - r / W) (B2 - B0)
(tests/numpy_restatement.py, _primary: the column over the HEIGHT, the row over the WIDTH), and the pixel's world point is
eye + z d.  Moving the previous eye by -z (k / H) (B1 - B0) + z (j / W) (B2 - B0) therefore shows the point of depth z at column
c + k and row r + j of the previous frame: the column shift divides by H, the row shift by W.  Widths and heights are powers of
two, colours are integers / 256, depths 8 or 16, sample counts such that n / tot = 1/2: all sums, products and quotients below are
dyadic numbers of a few bits, the same in float32 and float64.

The expectation (expected_sequence) solves the previous camera's 3 x 3 system by Cramer's rule for every pixel, spreads the
history with tent weights, drops -- selects away, never multiplies by 0 -- every tap outside the frame or refused by a stop, and
keeps the history where the remaining weight reaches min_weight.  Channel 10 is expected only where lum(C) and lum(hC) have the
same bits (CASE "still-colour"): the luminance weights are not dyadic."""
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64

B0, E1, E2 = np.array([-0.5, -0.25, -1.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
BASIS = np.concatenate([B0, B0 + E1, B0 + E2, B0 + E1 + E2]).astype(f32)
EYE = np.array([50.0, 52.0, 295.5])
P_EXACT = np.array([[0.0, 0.0, -1.0], [0.5, 0.0, -0.25], [0.0, 1.0, -0.25]], f32)  # the inverse of [B0 | E1 | E2], by hand
SIZES = [(64, 32), (32, 64), (16, 4)]  # (W, H): two that are not square and span several 32 x 8 workgroups, one inside one
N = 4
Z = 8.0
OPTS = dict(history_cap=256.0, depth_tol=2.0 ** -5, normal_tol=0.5, albedo_tol=2.0 ** -6, min_weight=0.25)
NORMAL, ALBEDO = (0.0, 0.0, 1.0), (0.5, 0.25, 0.75)


def shifts(W):
    """(k, j): whole pixels; halves and quarters of weights with taps at row or column -1; cc = -1; one surviving tap pair; none."""
    return [(3, 0), (0, 2), (-5, 1), (0.5, 0), (0, 0.5), (1.5, -0.5), (-0.5, -0.5), (-1, 0), (W - 0.5, 0), (W, 0)]


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def is_f32(a):
    a = np.asarray(a, f64)
    with np.errstate(all="ignore"):
        return bool(np.all((a.astype(f32).astype(f64) == a) | ~np.isfinite(a)))


def make_frame(W, H, seed, depth=Z):
    """Colour: integers 0..15 / 256; normal (0, 0, 1); albedo (0.5, 0.25, 0.75); channel 10: integers 1..8 / 1024; channels
    11-13 (which the stage must not touch): integers / 16."""
    rng = np.random.default_rng(seed)
    F = np.zeros((H, W, 14), f32)
    F[..., 0:3] = rng.integers(0, 16, (H, W, 3)) / 256.0
    F[..., 3:6], F[..., 6:9], F[..., 9] = NORMAL, ALBEDO, depth
    F[..., 10] = rng.integers(1, 9, (H, W)) / 1024.0
    F[..., 11:14] = rng.integers(0, 16, (H, W, 3)) / 16.0
    return F


def shifted_eye(W, H, k, j, eye=EYE, z=Z):
    """The eye from which the point that `eye` sees at depth z in pixel (r, c) lies in pixel (r + j, c + k)."""
    e = np.asarray(eye, f64) - z * (k / H) * E1 + z * (j / W) * E2
    assert is_f32(e), e
    return e


class Case:
    """calls: [(frame [H][W][14] float32, samples, basis[12], eye[3])] of ONE session with the options `opts`.
    expect[i]: what call i must return: "colour" float64 [H][W][3] or None (not exact: the model's bits decide), "counts"
    uint32 [H][W], "ch10" float32 [H][W] or None, "kept" bool [H][W].  share: the share of pixels with history that geometry
    predicts for the last call, or None.  pixels: [(call, row, column, "keep" | "restart")] stated by hand.
    finite: the calls whose channels 0-2 and 10 must be finite everywhere."""

    def __init__(self, name, W, H, calls, opts=None, exact=True, share=None, pixels=(), finite=(), differs=True):
        self.name, self.W, self.H = name, W, H
        self.calls = [(np.ascontiguousarray(F, f32), int(n), np.asarray(b, f32).reshape(12), np.asarray(e, f32).reshape(3)) for F, n, b, e in calls]
        self.opts = dict(OPTS, **(opts or {}))
        self.exact, self.share, self.pixels, self.finite, self.differs = exact, share, list(pixels), list(finite), differs
        self.expect = expected_sequence(W, H, self.calls, self.opts, exact)
        for F, _, _, _ in self.calls:
            F.setflags(write=False)

    def __repr__(self):
        return self.name


# ---- the independent expectation --------------------------------------------------------------------------------------

def reproject(W, H, basis, eye, prev_basis, prev_eye, z):
    """(t, row, column) in the previous camera of every pixel's world point, float64; NaN where it has none."""
    B, Pb = np.asarray(basis, f64).reshape(4, 3), np.asarray(prev_basis, f64).reshape(4, 3)
    r, c = (a.astype(f64) for a in np.mgrid[0:H, 0:W])
    sy, v = c / H, 1.0 - r / W  # the renderer's ray: the column over the height, the row over the width
    with np.errstate(all="ignore"):
        d = B[0] + sy[..., None] * (B[1] - B[0]) + v[..., None] * (B[2] - B[0])
        q = (np.asarray(eye, f64) + z[..., None] * d) - np.asarray(prev_eye, f64)
        m0, m1, m2 = Pb[0], Pb[1] - Pb[0], Pb[2] - Pb[0]  # X = eye' + t (m0 + sy' m1 + v' m2): Cramer's rule
        det = np.dot(m0, np.cross(m1, m2))
        t = (q @ np.cross(m1, m2)) / det
        t_sy = np.cross(q, m2) @ m0 / det
        t_v = np.cross(m1, q) @ m0 / det
        col, row = (t_sy / t) * H, (1.0 - t_v / t) * W
    seen = np.isfinite(z) & (z > 0) & np.isfinite(t) & (t > 0) & np.isfinite(row) & np.isfinite(col)
    nan = np.full((H, W), np.nan)
    return np.where(seen, t, nan), np.where(seen, row, nan), np.where(seen, col, nan)


def _gather(hist, F, basis, eye, W, H, opts):
    """(kept, hC, hs2 or None, hN) from the history's four tent-weighted neighbours of every pixel's previous position."""
    N_, A, z = F[..., 3:6], F[..., 6:9], F[..., 9]
    t, row, col = reproject(W, H, basis, eye, hist["basis"], hist["eye"], z)
    seen = np.isfinite(t)
    row0 = np.clip(np.floor(np.where(seen, row, 0.0)), -2, H + 1)
    col0 = np.clip(np.floor(np.where(seen, col, 0.0)), -2, W + 1)
    ws, sC, sN = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W))
    ss = np.zeros((H, W)) if hist["s2"] is not None else None
    for dr in (0, 1):
        for dc in (0, 1):
            tr, tc = row0 + dr, col0 + dc
            with np.errstate(all="ignore"):
                w = np.maximum(1.0 - np.abs(row - tr), 0.0) * np.maximum(1.0 - np.abs(col - tc), 0.0)
                inside = (tr >= 0) & (tr < H) & (tc >= 0) & (tc < W)
                ir, ic = np.clip(tr, 0, H - 1).astype(int), np.clip(tc, 0, W - 1).astype(int)
                dA = hist["A"][ir, ic] - A
                agree = ((np.abs(hist["z"][ir, ic] - t) <= opts["depth_tol"] * t)
                         & ((hist["N"][ir, ic] * N_).sum(-1) >= opts["normal_tol"]) & ((dA * dA).sum(-1) <= opts["albedo_tol"]))
            take = seen & inside & agree & (w > 0)  # everything else is left out, whatever it holds
            w = np.where(take, w, 0.0)
            ws += w
            sC += np.where(take[..., None], w[..., None] * np.where(take[..., None], hist["colour"][ir, ic], 0.0), 0.0)
            sN += np.where(take, w * hist["count"][ir, ic], 0.0)
            if ss is not None:
                ss += np.where(take, w * np.where(take, hist["s2"][ir, ic], 0.0), 0.0)
    kept = ws >= opts["min_weight"]
    safe = np.where(kept, ws, 1.0)
    hC = np.where(kept[..., None], sC / safe[..., None], 0.0)
    hN = np.where(kept, np.minimum(sN / safe, opts["history_cap"]), 0.0)
    return kept, hC, (np.where(kept, ss / safe, 0.0) if ss is not None else None), hN


def round_to_f32(q):
    """The float32 nearest to the rational q, by exact comparison."""
    a = f32(float(q))
    cands = [np.nextafter(a, f32(-np.inf)), a, np.nextafter(a, f32(np.inf))]
    errs = sorted((abs(Fraction(float(x)) - q), i) for i, x in enumerate(cands))
    assert errs[0][0] < errs[1][0], q  # (no tie)
    return cands[errs[0][1]]


def expected_sequence(W, H, calls, opts, exact=True):
    opts = {k: float(f32(v)) for k, v in opts.items()}
    hist, out = None, []
    for F32, n, basis, eye in calls:
        F = F32.astype(f64)
        C, s2c = F[..., 0:3], F[..., 10]
        ch10 = None
        if hist is None:
            kept, hC, hN = np.zeros((H, W), bool), np.zeros((H, W, 3)), np.zeros((H, W))
            ch10 = F32[..., 10].copy()
        else:
            kept, hC, hs2, hN = _gather(hist, F, basis, eye, W, H, opts)
        tot = hN + n
        with np.errstate(all="ignore"):
            colour = np.where(kept[..., None], hC + (n / tot)[..., None] * (C - hC), C)
        if hist is not None and exact and hs2 is not None and np.array_equal(np.where(kept[..., None], hC, C), C) and is_f32(hs2):
            # delta = lum(C) - lum(hC) is 0 with the same bits on both sides: one correctly rounded division is left
            ch10 = F32[..., 10].copy()
            for r_, c_ in np.argwhere(kept & (tot > 1)):
                hn = Fraction(float(hN[r_, c_]))
                num = Fraction(float(hs2[r_, c_])) * max(hn - 1, 0) + Fraction(float(s2c[r_, c_])) * (n - 1)
                assert is_f32(float(num)), num  # (the numerator is exact in float32, the quotient is the only rounding)
                ch10[r_, c_] = round_to_f32(num / (Fraction(float(tot[r_, c_])) - 1))
        if exact:
            assert is_f32(colour) and is_f32(tot), "the construction is not exact in float32"
        out.append(dict(colour=colour if exact else None, counts=np.floor(tot + 0.5).astype(np.uint32), ch10=ch10, kept=kept))
        hist = dict(colour=colour, s2=F[..., 10] if hist is None else (ch10.astype(f64) if ch10 is not None else None),
                    N=F[..., 3:6], z=F[..., 9], A=F[..., 6:9], count=tot, basis=basis, eye=eye)
    return out


def check(case, outs, counts, what):
    """outs [K][H][W][14] float32 and counts [K][H][W] of the case's calls, from the model or from the kernel, against the
    expectation: colour BITS and float64 values, counts, channel 10 where it is expected, the hand-stated pixels, finiteness, and
    channels 3-9 and 11-13 byte for byte as they went in."""
    for i, (e, (F, n, _, _)) in enumerate(zip(case.expect, case.calls)):
        got, cnt, tag = np.asarray(outs[i]), np.asarray(counts[i]), (what, case.name, i)
        assert got.dtype == f32 and got.shape == F.shape
        assert np.array_equal(got[..., 3:10].view(np.uint32), F[..., 3:10].view(np.uint32)), tag
        assert np.array_equal(got[..., 11:].view(np.uint32), F[..., 11:].view(np.uint32)), tag
        assert np.array_equal(cnt, e["counts"]), (tag, np.argwhere(cnt != e["counts"])[:5])
        if e["colour"] is not None:
            want = e["colour"].astype(f32)
            bad = np.argwhere(~((got[..., 0:3].view(np.uint32) == want.view(np.uint32)) | (np.isnan(got[..., 0:3]) & np.isnan(want))))
            assert bad.size == 0, (tag, len(bad), bad[:5], [(got[..., 0:3][tuple(b)], want[tuple(b)]) for b in bad[:5]])
            assert np.array_equal(got[..., 0:3].astype(f64), e["colour"], equal_nan=True), tag
        if e["ch10"] is not None:
            bad = np.argwhere(~((got[..., 10].view(np.uint32) == e["ch10"].view(np.uint32)) | (np.isnan(got[..., 10]) & np.isnan(e["ch10"]))))
            assert bad.size == 0, (tag, "channel 10", len(bad), bad[:5], [(got[..., 10][tuple(b)], e["ch10"][tuple(b)]) for b in bad[:5]])
        if i in case.finite:
            bad = np.argwhere(~np.isfinite(got[..., [0, 1, 2, 10]]))
            assert bad.size == 0, (tag, "not finite", len(bad), bad[:8])
    for i, r, c, state in case.pixels:
        n = case.calls[i][1]
        if state == "keep":
            assert counts[i][r, c] > n, (what, case.name, i, r, c, "must keep its history")
        else:
            assert counts[i][r, c] == n, (what, case.name, i, r, c, "must restart")
            assert np.array_equal(outs[i][r, c].view(np.uint32), case.calls[i][0][r, c].view(np.uint32)), (what, case.name, i, r, c, "its own values")


def check_inputs(case):
    """Conditions on the case itself, so that no comparison passes by comparing nothing."""
    last, (F, n, _, _) = case.expect[-1], case.calls[-1]
    share = float(last["kept"].mean())
    if case.share is not None:
        assert share == case.share, (case.name, share, case.share)
    assert np.array_equal(last["counts"] > n, last["kept"])
    if case.exact and case.differs:
        assert last["kept"].any() and not np.array_equal(last["colour"].astype(f32), F[..., 0:3], equal_nan=True), case.name
    for i, r, c, state in case.pixels:
        assert bool(case.expect[i]["kept"][r, c]) == (state == "keep"), (case.name, i, r, c, state)
    return share


# ---- part 1: reprojection ---------------------------------------------------------------------------------------------

def predicted_share(W, H, k, j):
    """Whole-pixel shifts: the overlap of the frame with itself moved by (k, j); (W - 0.5, 0): column 0 alone."""
    if k == W - 0.5 and j == 0:
        return 1.0 / W
    if float(k).is_integer() and float(j).is_integer():
        return max(W - abs(k), 0) * max(H - abs(j), 0) / (W * H)
    return None


def shift_case(W, H, k, j, depth=Z):
    """Two frames of unrelated colours; the second camera sees every point of depth 8 by (k, j) pixels from where the first did.
    With depth 16 in both frames the same two eyes move the image by half of that: X = eye + d z."""
    scale = Z / depth
    calls = [(make_frame(W, H, 11, depth), N, BASIS, shifted_eye(W, H, k, j)), (make_frame(W, H, 12, depth), N, BASIS, EYE)]
    return Case(f"{'shift' if depth == Z else 'parallax'}-{W}x{H}-k{k:g}-j{j:g}", W, H, calls, share=predicted_share(W, H, k * scale, j * scale),
                differs=k * scale < W)


def still_colour_case(W, H, k=-5, j=1):
    """A whole-pixel shift whose second frame shows the first frame's colours moved with it (other channel 10): lum(C) and
    lum(hC) have the same bits, delta is 0 and s2_out = (3 s2' + 3 s2c) / 7, one correctly rounded division."""
    F1, F2 = make_frame(W, H, 21), make_frame(W, H, 22)
    r, c = np.mgrid[0:H, 0:W]
    sr, sc = r + j, c + k
    inside = (sr >= 0) & (sr < H) & (sc >= 0) & (sc < W)
    F2[..., 0:3] = np.where(inside[..., None], F1[np.clip(sr, 0, H - 1), np.clip(sc, 0, W - 1), 0:3], F2[..., 0:3])
    case = Case(f"still-colour-{W}x{H}", W, H, [(F1, N, BASIS, shifted_eye(W, H, k, j)), (F2, N, BASIS, EYE)], share=predicted_share(W, H, k, j),
                differs=False)
    e = case.expect[-1]
    assert e["ch10"] is not None and np.array_equal(e["kept"], inside)
    assert not np.array_equal(e["ch10"], F2[..., 10])  # (and channel 10 does change)
    return case


def dolly_case():
    """32 x 64: the camera moves 8 back along its axis between a frame of depth 16 and one of depth 8, so the image shrinks
    to half about (row 12, column 8): alpha = 16 is not the pixel's own z.  A block of sky (z = 0) in the second frame has
    X = eye, which the previous camera sees at depth 8 in (row 24, column 16) -- and the history holds depth 8 exactly there:
    only `z > 0` keeps the sky from accumulating.  The block covers every pixel whose footprint touches that history pixel."""
    W, H = 32, 64
    F1, F2 = make_frame(W, H, 31, 16.0), make_frame(W, H, 32, 8.0)
    F1[24, 16, 9] = 8.0
    F2[20:29, 12:21, 9] = 0.0
    F2[40, 5, 9] = -0.0
    case = Case("dolly-32x64", W, H, [(F1, N, BASIS, EYE + np.array([0.0, 0.0, 8.0])), (F2, N, BASIS, EYE)],
                share=1.0 - 82.0 / (W * H), pixels=[(1, 24, 16, "restart"), (1, 20, 12, "restart"), (1, 40, 5, "restart"), (1, 0, 0, "keep"), (1, 63, 31, "keep")])
    return case


# ---- part 2: the stops at their thresholds ------------------------------------------------------------------------------

def threshold_case(W, H, k=0, j=0):
    """Single history pixels edited to sit on each stop's threshold and one float beyond it (depth_tol 2^-5 at alpha = 8:
    0.25; normal_tol 0.5; albedo_tol 2^-6: |dA| = 0.125); the camera at rest or shifted by whole pixels, every tap of weight 1."""
    F1, F2 = make_frame(W, H, 41), make_frame(W, H, 42)
    edits = [((1, 3), 9, 8.25, "keep"), ((1, 5), 9, 7.75, "keep"), ((2, 3), 9, up(8.25), "restart"), ((2, 5), 9, down(7.75), "restart"),
             ((0, 7), 5, 0.5, "keep"), ((0, 9), 5, down(0.5), "restart"),
             ((3, 6), 6, 0.625, "keep"), ((3, 8), 6, 0.375, "keep"), ((3, 10), 6, up(0.625), "restart"), ((3, 12), 6, down(0.375), "restart")]
    pixels = []
    for (r, c), ch, value, state in edits:
        F1[r, c, ch] = value
        pixels.append((1, r - j, c - k, state))
        pixels.append((1, r - j, c - k + 1, "keep"))  # (the neighbour is not touched)
    return Case(f"thresholds-{W}x{H}-k{k}-j{j}", W, H, [(F1, N, BASIS, shifted_eye(W, H, k, j)), (F2, N, BASIS, EYE)], pixels=pixels,
                share=predicted_share(W, H, k, j) - 5.0 / (W * H))


def min_weight_case(W, H, min_weight):
    """(1/2, 1/2) shift: the last row and column keep one tap pair (Ws = 1/2), the corner one tap (Ws = 1/4 exactly)."""
    calls = [(make_frame(W, H, 51), N, BASIS, shifted_eye(W, H, 0.5, 0.5)), (make_frame(W, H, 52), N, BASIS, EYE)]
    corner = "keep" if min_weight <= 0.25 else "restart"
    return Case(f"min-weight-{W}x{H}-{'at' if min_weight <= 0.25 else 'above'}", W, H, calls, opts=dict(min_weight=min_weight),
                pixels=[(1, H - 1, W - 1, corner), (1, H - 1, W - 2, "keep"), (1, H - 2, W - 1, "keep")],
                share=1.0 if corner == "keep" else 1.0 - 1.0 / (W * H))


def history_cap_case(W, H):
    """history_cap = 2 under a camera at rest: tot = 6 and k = 4/6 (not dyadic: the colour is the model's)."""
    calls = [(make_frame(W, H, 61 + i), N, BASIS, EYE) for i in range(3)]
    case = Case(f"history-cap-2-{W}x{H}", W, H, calls, opts=dict(history_cap=2.0), exact=False, share=1.0)
    assert all((e["counts"] == c).all() for e, c in zip(case.expect, (4, 6, 6)))
    return case


def samples_case(W, H):
    """samples 1, 4, 2 on one session under a camera at rest: totals 1, 5, 7; the single-sample frame has n - 1 = 0 in the
    variance merge, as a history of one sample has hN - 1 = 0."""
    frames = [make_frame(W, H, 71 + i) for i in range(3)]
    case = Case(f"samples-1-4-2-{W}x{H}", W, H, [(f, n, BASIS, EYE) for f, n in zip(frames, (1, 4, 2))], exact=False, share=1.0)
    assert all((e["counts"] == c).all() for e, c in zip(case.expect, (1, 5, 7)))
    return case


# ---- part 3: values that are not finite -----------------------------------------------------------------------------------

def poisoned_history_case(W, H, value, stop):
    """Half-column shift.  History pixel (2, 5) holds `value` (NaN or +Inf) in colour and channel 10 and fails a stop for
    every pixel (depth 64, or a NaN normal).  Pixels (2, 4) and (2, 5) lose one tap of weight 1/2 and keep the other; pixels
    (1, 4) and (1, 5) meet it with weight 0.  Nothing of `value` may come out."""
    F1, F2 = make_frame(W, H, 81), make_frame(W, H, 82)
    F1[2, 5, 0:3], F1[2, 5, 10] = value, value
    if stop == "depth":
        F1[2, 5, 9] = 64.0
    else:
        F1[2, 5, 3:6] = np.nan
    name = f"poisoned-{'nan' if np.isnan(value) else 'inf'}-{stop}-{W}x{H}"
    return Case(name, W, H, [(F1, N, BASIS, shifted_eye(W, H, 0.5, 0)), (F2, N, BASIS, EYE)], finite=[1], share=1.0,
                pixels=[(1, r, c, "keep") for r in (1, 2, 3) for c in (3, 4, 5, 6)])


def poisoned_frame_case(W, H):
    """Three frames, half a column apart, history_cap 4 (so that tot = 8 on every kept pixel).  The SECOND frame has a NaN depth
    at (1, 3), a NaN normal at (2, 7) and a NaN albedo component at (3, 11): those pixels restart with their own values, and in
    the third call their neighbours are formed from the taps that are left."""
    F = [make_frame(W, H, 91 + i) for i in range(3)]
    F[1][1, 3, 9], F[1][2, 7, 4], F[1][3, 11, 8] = np.nan, np.nan, np.nan
    eyes = [shifted_eye(W, H, 1.0, 0), shifted_eye(W, H, 0.5, 0), EYE]
    own = [(1, 3), (2, 7), (3, 11)]
    pixels = [(1, r, c, "restart") for r, c in own] + [(1, r, c + d, "keep") for r, c in own for d in (-1, 1)]
    pixels += [(2, r, c + d, "keep") for r, c in own for d in (-2, -1, 0, 1)]
    return Case(f"poisoned-frame-{W}x{H}", W, H, [(f, N, BASIS, e) for f, e in zip(F, eyes)], opts=dict(history_cap=4.0), finite=[0, 1, 2], pixels=pixels,
                share=1.0)


# ---- the lists ----------------------------------------------------------------------------------------------------------

def _all_cases():
    cases = []
    for W, H in SIZES:
        cases += [shift_case(W, H, k, j) for k, j in shifts(W)]
        cases += [shift_case(W, H, k, j, depth=16.0) for k, j in shifts(W)]
        cases.append(still_colour_case(W, H))
    cases.append(dolly_case())
    for W, H in [(16, 4), (64, 32)]:
        cases += [threshold_case(W, H), threshold_case(W, H, 3, 0), min_weight_case(W, H, 0.25), min_weight_case(W, H, up(0.25)),
                  history_cap_case(W, H), samples_case(W, H)]
    return cases


def _nonfinite_cases():
    cases = []
    for W, H in [(16, 4), (32, 64)]:
        cases += [poisoned_history_case(W, H, v, s) for v in (np.nan, np.inf) for s in ("depth", "normal")]
        cases.append(poisoned_frame_case(W, H))
    return cases


CASES = _all_cases()
NONFINITE = _nonfinite_cases()
STREAMED = ["shift-64x32-k1.5-j-0.5", "parallax-32x64-k-5-j1"]  # the two that the GPU test also sends through enqueue_frames
