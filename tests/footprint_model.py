"""primary_candidates (csrc/pt_footprint.h) in NumPy float32: which spheres may a pixel's primary rays meet?  Vectorised over the
pixels of a tile, one ufunc per IEEE operation in the code's own order, no contraction; the per-sphere loops stay loops.  Neither
side uses a transcendental, square roots and divisions are IEEE on both, so tests/test_primary_exclusion_gpu.py requires the
device's words to EQUAL this model's, and tests/test_primary_exclusion_host.py proves the model sound against the reference's
intersection.  radius_factor and margin are the two constants of the argument (kFootprintRadiusFactor, kFootprintMargin): the
deliberately unsound builds PT_FOOTPRINT_MUTANT=1 / 2 are radius_factor=0.3 / margin=0.93."""
import numpy as np

f32 = np.float32
RADIUS_FACTOR, MARGIN = 1.05, 1.07

# The two extreme values the project's uniform can return (csrc/pt_device.h, uniform_from_u32: fmaf((float)x, c, c / 2) with
# c = 2.3283064e-10f; (float)0xFFFFFFFF = 2^32): one rounding of the exact value.
_C = f32(2.3283064e-10)
UNIFORM_MIN = f32(np.float64(_C) / 2.0)
UNIFORM_MAX = f32(4294967296.0 * np.float64(_C) + np.float64(_C) / 2.0)


def _dot(a, b):  # pt_device.h dot: a.x*b.x + a.y*b.y + a.z*b.z, left to right
    return ((a[0] * b[0]).astype(f32) + (a[1] * b[1]).astype(f32)).astype(f32) + (a[2] * b[2]).astype(f32)


def _lerp(a, b, t):  # pt_device.h lerp: a + (b - a) * t
    return [(a[k] + ((b[k] - a[k]).astype(f32) * t).astype(f32)).astype(f32) for k in range(3)]


def dir_at(basis, width, height, sx, sy):
    """The kernels' dir_at (pixel_kernel, the split kernel, pt_fast.hip): the primary direction for screen position (sx, sy) in
    PIXEL units.  (Power-of-two images multiply by the exact reciprocal there: the same float as this division.)"""
    B = [[np.full(np.shape(sx), f32(basis[3 * j + k]), dtype=f32) for k in range(3)] for j in range(4)]
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (np.asarray(sx, dtype=f32) / f32(height)).astype(f32)
        sy = (np.asarray(sy, dtype=f32) / f32(width)).astype(f32)
        return _lerp(_lerp(B[0], B[1], sy), _lerp(B[2], B[3], sy), (f32(1.0) - sx).astype(f32))


def tile_pixels(width, row_begin, row_end):
    """(row, col) as float32 of every tile pixel in the pixel kernels' order: tp -> row_begin + tp / width, tp % width"""
    tp = np.arange((row_end - row_begin) * width, dtype=np.int64)
    return (row_begin + tp // width).astype(f32), (tp % width).astype(f32)


def jittered_dir(basis, width, height, row, col, jx, jy):
    """primary_ray of the pixel kernels (src/pathtrace.cu:221-229) for the jitter draws (jx, jy)"""
    sx = (row + ((jx * f32(1.0)).astype(f32) - f32(0.5)).astype(f32)).astype(f32)
    sy = (col + ((jy * f32(1.0)).astype(f32) - f32(0.5)).astype(f32)).astype(f32)
    return dir_at(basis, width, height, sx, sy)


def five_dirs(basis, width, height, row, col):
    """Centre and the four corners, in the order both analyses evaluate them: [5][3] arrays over the pixels"""
    out = [dir_at(basis, width, height, row, col)]
    for k in range(4):
        out.append(dir_at(basis, width, height, (row + f32(0.5 if k & 1 else -0.5)).astype(f32), (col + f32(0.5 if k & 2 else -0.5)).astype(f32)))
    return out


def primary_candidates(spheres, eye, basis, width, height, row_begin, row_end, radius_factor=RADIUS_FACTOR, margin=MARGIN):
    """Returns a dict: "word" uint32 per tile pixel (bit j = sphere j is kept), the per-rule drop masks "A", "B", "C_out" (an
    outside sphere farther than the wall), "C_wall" (a tame wall farther than the wall) as uint32 words, "keep_all_n" (bool: the
    n > 16 || n < 2 shortcut), "keep_all_coarse" (bool per pixel: the early return), "rho", and "near" (bool per pixel: some
    (pixel, sphere) pair lies within `near_rho` footprint radii of rule (A)'s or (B)'s threshold or within `near_c` of (C)'s)."""
    n = len(spheres)
    row, col = tile_pixels(width, row_begin, row_end)
    npx = row.size
    all_bits = np.uint32(0xFFFFFFFF if n >= 32 else (1 << n) - 1)
    zero_w = np.zeros(npx, dtype=np.uint32)
    out = {"word": np.full(npx, all_bits, dtype=np.uint32), "A": zero_w.copy(), "B": zero_w.copy(), "C_out": zero_w.copy(),
           "C_wall": zero_w.copy(), "keep_all_n": n > 16 or n < 2, "keep_all_coarse": np.zeros(npx, dtype=bool),
           "rho": np.zeros(npx, dtype=f32), "near": np.zeros(npx, dtype=bool)}
    if n > 16 or n < 2:
        return out
    fac, mar = f32(radius_factor), f32(margin)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d5 = five_dirs(basis, width, height, row, col)
        dc = d5[0]
        lc = np.sqrt(_dot(dc, dc)).astype(f32)
        dev, dmax = np.zeros(npx, dtype=f32), lc
        for k in range(4):
            e = [(d5[1 + k][i] - dc[i]).astype(f32) for i in range(3)]
            dev = np.fmax(dev, np.sqrt(_dot(e, e)).astype(f32))          # fmaxf: a NaN operand loses
            dmax = np.fmax(dmax, np.sqrt(_dot(d5[1 + k], d5[1 + k])).astype(f32))
        dmax = (dmax * f32(1.000001)).astype(f32)
        dmin = ((lc - dev).astype(f32) * f32(0.999999)).astype(f32)
        rho = (((fac * dev).astype(f32) / lc).astype(f32) + f32(1e-6)).astype(f32)
        coarse = ~(rho <= f32(0.00390625)) | ~(dmin > 0) | ~(lc > 0)     # NaN, degenerate or coarse footprint: keep all
        inv = (f32(1.0) / lc).astype(f32)
        u = [(dc[i] * inv).astype(f32) for i in range(3)]
        ex, ey, ez = f32(eye[0]), f32(eye[1]), f32(eye[2])

        def operands(j):  # stage_scene: off and c of src/pathtrace.cu:73,76 for a ray from the eye
            p, r0 = spheres["pos"][j].astype(f32), f32(spheres["radius"][j])
            rr = f32(r0 * r0)
            off1 = [f32(ex - p[0]), f32(ey - p[1]), f32(ez - p[2])]
            o2 = f32(f32(f32(off1[0] * off1[0]) + f32(off1[1] * off1[1])) + f32(off1[2] * off1[2]))
            c = f32(o2 - rr)
            off = [np.full(npx, off1[i], dtype=f32) for i in range(3)]
            return off, o2, c, rr, np.sqrt(rr).astype(f32)

        # pass 1: the reference wall W
        Uw = np.full(npx, np.inf, dtype=f32)
        dist_c, tame = [None] * n, [None] * n
        w_idx = np.full(npx, -1, dtype=np.int64)
        for j in range(n):
            off, o2, c, rr, r = operands(j)
            hu = _dot(u, off)
            tame[j] = np.zeros(npx, dtype=bool)
            dist_c[j] = np.zeros(npx, dtype=f32)
            if c <= f32(-o2 * f32(0.000244140625)):                      # eye robustly inside
                sq = np.sqrt(((hu * hu).astype(f32) - c).astype(f32)).astype(f32)
                dist = np.where(hu > 0, (f32(-c) / (sq + hu).astype(f32)).astype(f32), (sq - hu).astype(f32))
                cp = (sq / r).astype(f32)
                bend = (rho * (f32(1.0) + ((f32(2.5) * dist).astype(f32) / (r * cp).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                ok = (cp >= (f32(100.0) * rho).astype(f32)) & (bend <= (f32(0.5) * cp).astype(f32)) & (dist > 0)
                tame[j], dist_c[j] = ok, dist
                U = ((dmax * f32(1.0203)).astype(f32) * dist).astype(f32)
                take = ok & (((f32(1.0203) * dist).astype(f32) / dmin).astype(f32) < f32(900000.0)) & (U < Uw)
                Uw = np.where(take, U, Uw)
                w_idx = np.where(take, j, w_idx)
        # pass 2: drop what provably cannot be returned
        keep = zero_w.copy()
        mUw = (mar * Uw).astype(f32)
        near = np.zeros(npx, dtype=bool)
        for j in range(n):
            off, o2, c, rr, r = operands(j)
            hu = _dot(u, off)
            bit = np.uint32(1 << j)
            dA = dB = dCo = dCw = np.zeros(npx, dtype=bool)
            if c >= f32(o2 * f32(0.00390625)):                           # eye robustly outside
                lo = np.sqrt(o2).astype(f32)
                cosc = ((np.abs(hu) / lo).astype(f32) + rho).astype(f32)
                rhsA = f32(f32(c / o2) * f32(0.999755859375))
                dA = (cosc * cosc).astype(f32) <= rhsA                   # (A) missed
                rl = (rho * lo).astype(f32)
                dB = hu > (rl * f32(1.000001)).astype(f32)               # (B) behind
                lhsC = ((dmin * f32(lo - r)).astype(f32) * f32(0.9990234375)).astype(f32)
                dCo = lhsC >= mUw                                        # (C) farther than W
                near |= np.abs((np.abs(hu) / lo).astype(np.float64) - np.sqrt(np.float64(c) / np.float64(o2))) <= NEAR_RHO * rho
                near |= np.abs(hu) <= NEAR_RHO * rl
                near |= np.isfinite(mUw) & (np.minimum(lhsC, mUw) * NEAR_C >= np.maximum(lhsC, mUw))
            else:
                lhsC = ((dmin * dist_c[j]).astype(f32) * f32(f32(1.0) / f32(1.0203))).astype(f32)
                dCw = tame[j] & (lhsC >= mUw)                            # (C)
                near |= tame[j] & np.isfinite(mUw) & (w_idx != j) & (np.minimum(lhsC, mUw) * NEAR_C >= np.maximum(lhsC, mUw))
            drop = dA | dB | dCo | dCw
            keep |= np.where(drop, np.uint32(0), bit)
            for name, m in (("A", dA), ("B", dB), ("C_out", dCo), ("C_wall", dCw)):
                out[name] |= np.where(m & ~coarse, bit, np.uint32(0))
    out["word"] = np.where(coarse, all_bits, keep).astype(np.uint32)
    out["keep_all_coarse"] = coarse
    out["rho"] = rho
    out["near"] = near & ~coarse
    return out


# "near a rule's threshold", from the model's own quantities: (A) the centre direction's |cos angle(u_c, off)| within NEAR_RHO
# footprint radii of the silhouette's sqrt(c / |off|^2); (B) |u_c . off| within NEAR_RHO rho |off| of zero; (C) the two sides of the
# comparison within a factor NEAR_C.  A radius factor of 0.3 moves (A) and (B) by 0.75 rho and a margin of 0.93 moves (C) by 13 %.
NEAR_RHO = 4.0
NEAR_C = f32(1.2)
