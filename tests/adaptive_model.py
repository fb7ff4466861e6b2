"""NumPy restatement of adaptive sampling's decision (include/ptcore.h, pt_progressive_set_adaptive; EXACTNESS.md A.20), for the
tests: which pixels a session's next pass renders, from the frame at the session's count and the record's two counts."""
import numpy as np


def luminance(c0, c1, c2):
    """pt_device.h luminance(): the reference's literals in double, rounded to float (pathtrace.cu:67-69)."""
    d = 0.2126 * c0.astype(np.float64) + 0.7152 * c1.astype(np.float64)
    return (d + 0.0722 * c2.astype(np.float64)).astype(np.float32)


def converged(frame, n0, n1, n, tolerance, floor):
    """frame [rows][width][14] float32 at n samples; n0, n1 [rows][width] the record's colour and first-hit counts."""
    lum = luminance(frame[..., 0], frame[..., 1], frame[..., 2]).astype(np.float64)
    tol = np.float64(np.float32(tolerance))
    m = np.maximum(lum, np.float64(np.float32(floor)))
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
