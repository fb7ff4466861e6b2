"""NumPy restatement of adaptive sampling's decision (include/ptcore.h, pt_progressive_set_adaptive; EXACTNESS.md A.20), for the
tests: which pixels a session's next pass renders, from the frame at the session's count and the record's two counts."""
import numpy as np


def luminance(c0, c1, c2):
    """pt_device.h luminance(): the reference's literals in double, rounded to float (pathtrace.cu:67-69)."""
    d = 0.2126 * c0.astype(np.float64) + 0.7152 * c1.astype(np.float64)
    return (d + 0.0722 * c2.astype(np.float64)).astype(np.float32)


def converged(frame, n0, n1, n, tolerance, floor):
    """frame [rows][width][14] float32 at n samples; n0, n1 [rows][width] the record's colour and first-hit counts."""
    with np.errstate(all="ignore"):
        lum = luminance(frame[..., 0], frame[..., 1], frame[..., 2]).astype(np.float64)
        tol = np.float64(np.float32(tolerance))
        fl = np.float64(np.float32(floor))
        # the header's max as C evaluates it, lum > floor ? lum : floor: a NaN luminance takes the floor (np.maximum would keep it)
        m = np.where(lum > fl, lum, fl)
        # (a NaN variance compares false: never converged)
        b = (n0 == n) & (frame[..., 10].astype(np.float64) <= ((tol * tol) * np.float64(n)) * (m * m))
    return (n1 == 0) | b


def dilate(unconv, radius):
    """True where some unconverged pixel lies in the (2 radius + 1)^2 window, clipped to the tile."""
    rows, w = unconv.shape
    out = np.zeros_like(unconv)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            src = unconv[max(0, dy):rows + min(0, dy), max(0, dx):w + min(0, dx)]
            out[max(0, -dy):rows + min(0, -dy), max(0, -dx):w + min(0, -dx)] |= src
    return out


def next_active(active, frame, n0, n1, n, tolerance, floor, min_samples, radius):
    """The set the next pass renders, given the set of the last pass and the session's count n."""
    if n < min_samples:
        return active.copy()
    unconv = active & ~converged(frame, n0, n1, n, tolerance, floor)
    return active & dilate(unconv, radius)


# ---- the record, and one whole call of the selection (csrc/pt_kernel.h, pt_launch_adaptive_select) -----------------------------

REC_WORDS, REC_N_COLOR, REC_N_HIT, REC_M2 = 26, 10, 11, 13  # PT_CHUNK_WORDS, PT_REC_* (csrc/pt_kernel.h)
BLOCK = 256  # PT_ADAPTIVE_BLOCK


def frame_from_record(rec, counts):
    """The 14 channels of every pixel at its own count (frame_values, csrc/pt_scene_lds.h): rec [26][pixels] uint32, counts
    [pixels]; float32 [pixels][14].  Channels 0-9 = sum / (float)count; 10-13 = M2 / (float)(n_k - 1) where the accumulator's
    count n_k (word 10 for the colour, word 11 for normal, albedo and depth) is >= 2, else 0.  All in float32."""
    rec = np.asarray(rec, np.uint32)
    f = rec.view(np.float32)
    out = np.zeros((rec.shape[1], 14), np.float32)
    with np.errstate(all="ignore"):
        cnt = np.asarray(counts).astype(np.int32).astype(np.float32)
        for c in range(10):
            out[:, c] = f[c] / cnt
        for k in range(4):
            nk = rec[REC_N_COLOR if k == 0 else REC_N_HIT].view(np.int32)
            den = (np.where(nk >= 2, nk, 2) - 1).astype(np.float32)
            out[:, 10 + k] = np.where(nk >= 2, f[REC_M2 + 2 * k] / den, np.float32(0))
    return out


def select(rec, width, n, n_end, mode, peek, tolerance, floor, min_samples, radius, mask, counts, lst, words):
    """What one call of the selection must leave behind: (mask, counts, list, words, block prefix, next set).  mode 0 = the rule
    on the pixels of mask bit 0 (once n >= min_samples), 1 = mask bit 0 as it is, 2 = every pixel.  Not peek: the list is the new
    set in raster order over words[0] entries and untouched behind them, the set's counts become n_end, the mask is the set as
    0 / 1, words[1] = n_end unless the set is empty.  Peek: only words[0], the prefix and the mask's bits above bit 0 are the
    call's (mode 2 makes bit 0 of every pixel 1: that IS the mode's set); the mask returned for a peek holds bit 0 only."""
    rec = np.asarray(rec, np.uint32)
    tp = rec.shape[1]
    mask, counts = np.asarray(mask, np.uint8).reshape(-1), np.asarray(counts, np.uint32).reshape(-1).copy()
    lst, words = np.asarray(lst, np.uint32).reshape(-1).copy(), np.asarray(words, np.uint32).reshape(-1).copy()
    rows = tp // width
    assert rows * width == tp and n_end > n >= 0
    act = np.ones(tp, bool) if mode == 2 else (mask & 1) != 0
    unconv = act
    if mode == 0 and n >= min_samples:
        frame = frame_from_record(rec, np.full(tp, n))
        unconv = act & ~converged(frame, rec[REC_N_COLOR], rec[REC_N_HIT], np.uint32(n), tolerance, floor)
    new = act & dilate(unconv.reshape(rows, width), radius).reshape(-1)
    per_block = np.add.reduceat(new.astype(np.uint32), np.arange(0, tp, BLOCK))
    prefix = (np.cumsum(per_block, dtype=np.uint64) - per_block).astype(np.uint32)
    idx = np.flatnonzero(new).astype(np.uint32)
    words[0] = idx.size
    if peek:
        return act.astype(np.uint8), counts, lst, words, prefix, new
    lst[:idx.size] = idx
    counts[new] = n_end
    if idx.size:
        words[1] = n_end
    return new.astype(np.uint8), counts, lst, words, prefix, new
