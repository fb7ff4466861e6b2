"""NumPy restatement of the temporal accumulator (include/ptcore.h, pt_temporal_*; DENOISER.md, "Temporal accumulation"), for
the tests.  Written from the definition: the host step in float64, the per-pixel steps in float32, one rounding per operation
in the order the definition writes them, so the GPU kernel is held to it bit for bit."""
import numpy as np

import filter_model as fm

f32, f64 = np.float32, np.float64
DEFAULTS = dict(history_cap=256.0, depth_tol=0.02, normal_tol=0.9, albedo_tol=0.01, min_weight=0.25)


def camera_matrix(basis):
    """pt_temporal_camera: P = inverse of [B0 | B1-B0 | B2-B0] by cofactors in float64, entries rounded to float32.
    ValueError for a basis the C ABI refuses (no finite non-zero determinant, not a parallelogram)."""
    B = np.asarray(basis, dtype=f32).reshape(4, 3).astype(f64)
    m = np.stack([B[0], B[1] - B[0], B[2] - B[0]], axis=1)  # columns
    with np.errstate(all="ignore"):
        C = np.empty((3, 3), dtype=f64)
        C[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
        C[0, 1] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
        C[0, 2] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
        C[1, 0] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]
        C[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]
        C[1, 2] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]
        C[2, 0] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
        C[2, 1] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
        C[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        det = (m[0, 0] * C[0, 0] + m[0, 1] * C[0, 1]) + m[0, 2] * C[0, 2]
        if not np.isfinite(det) or det == 0.0:
            raise ValueError("basis: no finite non-zero determinant")
        tol = 1e-3 * np.sqrt((B[0, 0] * B[0, 0] + B[0, 1] * B[0, 1]) + B[0, 2] * B[0, 2])
        gap = np.abs(((B[1] + B[2]) - B[0]) - B[3])
        if not (gap <= tol).all():
            raise ValueError("basis: not a parallelogram")
        return (C.T / det).astype(f32)


def _lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class TemporalModel:
    """One session: accumulate(frame, n, basis, eye) -> (frame after the stage, uint32 counts), state carried to the next call."""

    def __init__(self, width, height, history_cap=256.0, depth_tol=0.02, normal_tol=0.9, albedo_tol=0.01, min_weight=0.25):
        self.W, self.H = width, height
        self.cap, self.depth_tol, self.normal_tol = f32(history_cap), f32(depth_tol), f32(normal_tol)
        self.albedo_tol, self.min_weight = f32(albedo_tol), f32(min_weight)
        self.hist = None  # ({colour, s2}, {normal, z}, {albedo, count}) each [H][W][4] float32
        self.P = self.eye = None

    def reset(self):
        self.hist = None

    def _gather(self, C, N, A, z, basis, eye):
        """Steps 3-5: (hC, hs2, hN) of every pixel."""
        H, W = self.H, self.W
        B = np.asarray(basis, dtype=f32).reshape(4, 3)
        eye = np.asarray(eye, dtype=f32).reshape(3)
        r = np.arange(H, dtype=f32)[:, None] * np.ones((1, W), dtype=f32)
        c = np.ones((H, 1), dtype=f32) * np.arange(W, dtype=f32)[None, :]
        sy = c / f32(H)
        v = f32(1.0) - r / f32(W)
        e1, e2 = B[1] - B[0], B[3] - B[2]
        X = []
        for k in range(3):
            a = B[0, k] + sy * e1[k]
            b = B[2, k] + sy * e2[k]
            d = a + v * (b - a)
            X.append(eye[k] + d * z)
        q = [X[k] - self.eye[k] for k in range(3)]
        P = self.P
        al, be, ga = ((P[i, 0] * q[0] + P[i, 1] * q[1]) + P[i, 2] * q[2] for i in range(3))
        cc = (be / al) * f32(H)  # (the column scales by H, the row by W: the reference divides the row by the width)
        rr = (f32(1.0) - ga / al) * f32(W)
        ok = (z > 0) & (al > 0) & (cc > f32(-1.0)) & (cc < f32(W)) & (rr > f32(-1.0)) & (rr < f32(H))
        rr, cc = np.where(ok, rr, f32(0.0)), np.where(ok, cc, f32(0.0))
        r0f, c0f = np.floor(rr), np.floor(cc)
        fr, fc = rr - r0f, cc - c0f
        r0, c0 = r0f.astype(np.int64), c0f.astype(np.int64)
        h0, h1, h2 = self.hist
        Ws = np.zeros((H, W), dtype=f32)
        sC = np.zeros((H, W, 3), dtype=f32)
        ss2 = np.zeros((H, W), dtype=f32)
        sN = np.zeros((H, W), dtype=f32)
        dtol = self.depth_tol * al
        for dr in (0, 1):
            for dc in (0, 1):
                tr, tc = r0 + dr, c0 + dc
                inside = (tr >= 0) & (tr < H) & (tc >= 0) & (tc < W)
                trc, tcc = np.clip(tr, 0, H - 1), np.clip(tc, 0, W - 1)
                t0, t1, t2 = h0[trc, tcc], h1[trc, tcc], h2[trc, tcc]
                w = (fr if dr else f32(1.0) - fr) * (fc if dc else f32(1.0) - fc)
                dA = t2[..., :3] - A
                valid = (ok & inside & (t2[..., 3] > 0) & (np.abs(t1[..., 3] - al) <= dtol)
                         & (_dot3(t1[..., :3], N) >= self.normal_tol) & (_dot3(dA, dA) <= self.albedo_tol))
                # an invalid tap contributes 0 to every sum: its values are selected away with its weight (0 * NaN is NaN)
                w = np.where(valid, w, f32(0.0)).astype(f32)
                t0 = np.where(valid[..., None], t0, f32(0.0)).astype(f32)
                tn = np.where(valid, t2[..., 3], f32(0.0)).astype(f32)
                Ws = Ws + w
                sC = sC + w[..., None] * t0[..., :3]
                ss2 = ss2 + w * t0[..., 3]
                sN = sN + w * tn
        keep = Ws >= self.min_weight
        hC = np.where(keep[..., None], sC / Ws[..., None], f32(0.0)).astype(f32)
        hs2 = np.where(keep, ss2 / Ws, f32(0.0)).astype(f32)
        hN = np.where(keep, np.minimum(sN / Ws, self.cap), f32(0.0)).astype(f32)
        return hC, hs2, hN

    def accumulate(self, frame, n, basis, eye):
        H, W = self.H, self.W
        F = np.array(frame, dtype=f32).reshape(H, W, 14)
        P = camera_matrix(basis)
        eye = np.asarray(eye, dtype=f32).reshape(3)
        n = f32(n)
        C, N, A, z, s2c = F[..., 0:3], F[..., 3:6], F[..., 6:9], F[..., 9], F[..., 10]
        with np.errstate(all="ignore"):
            if self.hist is None:
                hC, hs2, hN = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
            else:
                hC, hs2, hN = self._gather(C, N, A, z, basis, eye)
            tot = hN + n
            k = n / tot
            C_out = hC + k[..., None] * (C - hC)
            delta = _lum(C) - _lum(hC)
            merged = ((hs2 * np.maximum(hN - f32(1.0), f32(0.0)) + s2c * (n - f32(1.0))) + delta * delta * (hN * n / tot)) / (tot - f32(1.0))
            s2_out = np.where((hN > 0) & (tot > f32(1.0)), merged, s2c).astype(f32)
            counts = np.floor(tot + f32(0.5)).astype(np.uint32)
        assert C_out.dtype == f32 and s2_out.dtype == f32 and tot.dtype == f32
        out = F.copy()
        out[..., 0:3], out[..., 10] = C_out, s2_out
        self.hist = (np.concatenate([C_out, s2_out[..., None]], -1), np.concatenate([N, z[..., None]], -1),
                     np.concatenate([A, tot[..., None]], -1))
        self.P, self.eye = P, eye
        return out, counts


def accumulate_sequence(frames, n, bases, eyes, **opts):
    """Every frame of a sequence through one session: (frames after the stage [K][H][W][14], counts [K][H][W])."""
    frames = np.asarray(frames, dtype=f32)
    m = TemporalModel(frames.shape[2], frames.shape[1], **opts)
    outs, counts = zip(*(m.accumulate(f, n, b, e) for f, b, e in zip(frames, bases, eyes)))
    return np.stack(outs), np.stack(counts)


def run_calls(width, height, calls, **opts):
    """calls [(frame, samples, basis, eye)] through one session: ([frame after the stage], [counts])."""
    m = TemporalModel(width, height, **opts)
    outs, counts = zip(*(m.accumulate(f, n, b, e) for f, n, b, e in calls))
    return list(outs), list(counts)


# static camera, 4 x 4 spp against 16 spp: the worst |d| / (|ref| + 1e-3) measured with the committed model on the oracle's frames
# (colour: absolute 4.5e-6), and the bound: 4 x that, headroom for another summation order
RECORDED_COLOUR, RECORDED_VARIANCE = 3.0e-3, 4.3e-3
STATIC_FACTOR = 4.0
STATIC_SHARE = 0.75


def fly_pose(k):
    """Pose k of the fly-through the stage was prototyped on: 1.5 / 0 / -2.0 units and 0.7 degrees of yaw per frame."""
    return (50.0 + 1.5 * k, 52.0, 295.6 - 2.0 * k), -90.0 + 0.7 * k


def static_check(acc, counts, ref, what):
    """The static-camera condition and bounds, shared with the GPU test: at least 0.75 of the pixels reached count 16 and on
    those colour and channel 10 agree with the 16-spp frame."""
    full = counts == 16
    share = float(full.mean())
    colour = fm.rel_err(acc[full][:, 0:3], ref[full][:, 0:3])
    variance = fm.rel_err(acc[full][:, 10], ref[full][:, 10])
    print(f"STATIC {what}: share {share:.4f}, colour {colour:.3e} (absolute "
          f"{np.abs(acc[full][:, 0:3].astype(np.float64) - ref[full][:, 0:3]).max():.3e}), variance {variance:.3e}")
    assert share >= STATIC_SHARE
    assert colour <= STATIC_FACTOR * RECORDED_COLOUR
    assert variance <= STATIC_FACTOR * RECORDED_VARIANCE
