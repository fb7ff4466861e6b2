"""Float64 model of the fast mode's first hit (csrc/pt_fast.hip: sphere_t, nearest), the checks that hold a set of rays to
it, a float32 emulation of sphere_t, and the cases the host and GPU tests share.

THE MODEL of one ray against one sphere.  Inputs are float32: the origin o, the direction d, the centre g and r2 = fl32(r * r)
(what SceneLds::geom.w holds).  off = fl32(o - g) is the one rounding shared with the kernel; everything after it is float64:
a = d.d, h = d.off, c = |off|^2 - r2, disc = h^2 - a c, roots (-h -+ sqrt(disc)) / a (formed without cancellation), and t is
the reference's choice (pathtrace.cu:82-88,99): the smaller root if both are > 0, else the positive one, else none, accepted
if 0 < t < 1e6.  With eps = 2^-24, S_c = |off|^2 + r2, S_h = sum |d_i off_i| and K = 8:

    tol(t) = K eps [ (S_c + 2 |t| S_h + t^2 a) / (2 sqrt(disc)) + |t| ] + 2^ib ulp32(t)
    E_disc = K eps (2 |h| S_h + a S_c)

The first term of tol is the first-order effect on a root of the roundings in c, h and a (three-term fma chains: <= 3 eps of
their absolute sums), the second the last few operations (v_sqrt_f32 and v_rcp_f32 are 1-ulp instructions), the third the
truncation of the ranking key (ib = its index width; 0 where plain compares rank).  K counts roundings with room to spare --
it is not fitted to the kernel; the spare room also takes the two or three roundings of a primary direction (the kernel and
the reference interpolate d in float32, each in its own order; rays_of() rounds the exact interpolation once).

A pair is a SURE HIT if disc > 4 E_disc and its t > tol, a SURE MISS if disc < -4 E_disc or both roots < -tol, else a MAYBE.
Only the CHOSEN root is asked to clear its tol: a near root the float64 arithmetic finds negative is taken as negative.  (tol
is generous there by design -- K eps S_c is five times the three roundings of |off|^2 that really reach c -- and every
secondary ray starts 0.05 inside a sphere of radius 1e5, where that near root is -0.05 / cos and K eps S_c / (2 sqrt(disc)) is
0.048 / cos: asking it to clear tol as well would leave a fifth of all secondary rays undecided for no rounding that exists.)
An origin exactly on the sphere (c == 0) heading inward (h < 0) is a sure hit at t = -2 h / a; heading outward or along the
tangent (h >= 0) it is a maybe (the reference's own double square root can leave the zero root a few ulps above zero).  A t
within tol of the 1e6 limit is a maybe.  Per ray the answer is the sure hit of smallest t; the ray is DECIDED if no sphere is
a maybe and no other sphere's t - tol lies below the winner's t + tol, else UNDECIDED with the set of spheres that could win.

For the weak check a MAYBE pair whose discriminant is not surely positive gets a bound of its own around the double root
-h / a: the kernel only returns a root when ITS disc' >= 0, and |disc' - disc| <= 4 E_disc by the classification above, so
sqrt(disc') <= sqrt(max(disc, 0) + 4 E_disc) and |t - (-h / a)| <= sqrt(max(disc, 0) + 4 E_disc) / a + K eps (S_h / a + |t|)
+ 2^ib ulp32(t)."""
import numpy as np

EPS = 2.0 ** -24
K = 8.0
T_MAX = 1.0e6


def ulp32(t):
    return np.spacing(np.abs(np.asarray(t, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def index_bits(n):
    """ib of nearest<> for a scene of n spheres: 32 - clz(max(n - 1, 1)) up to 64 spheres, 0 on the compare path."""
    return 0 if n > 64 else max(n - 1, 1).bit_length()


def geometry(spheres):
    """(centres float32 [n][3], radii float32 [n], r2 = fl32(r * r) [n]) of a sphere table."""
    g = np.ascontiguousarray(spheres["pos"], dtype=np.float32)
    r = np.ascontiguousarray(spheres["radius"], dtype=np.float32)
    return g, r, (r * r).astype(np.float32)


class Pairs:
    """Every ray against every sphere: [rays][spheres] arrays."""

    def __init__(self, o, d, g, r2, ib):
        o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3), np.asarray(d, dtype=np.float32).reshape(-1, 3)
        off = (o[:, None, :] - g[None, :, :]).astype(np.float32).astype(np.float64)  # the shared rounding
        d64 = d.astype(np.float64)[:, None, :]
        r2 = r2.astype(np.float64)[None, :]
        a = (d64 * d64).sum(-1)
        h = (d64 * off).sum(-1)
        s_h = np.abs(d64 * off).sum(-1)
        off2 = (off * off).sum(-1)
        c, s_c = off2 - r2, off2 + r2
        disc = h * h - a * c
        sq = np.sqrt(np.maximum(disc, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = -(h + np.copysign(sq, h))
            t_big = q / a
            t_small = np.where(q != 0.0, c / np.where(q != 0.0, q, 1.0), 0.0)
            t_big = np.where(q != 0.0, t_big, 0.0)
            lo, hi = np.minimum(t_big, t_small) + 0.0, np.maximum(t_big, t_small) + 0.0
            key = (2.0 ** ib)

            def tol(t):
                return K * EPS * ((s_c + 2.0 * np.abs(t) * s_h + t * t * a) / (2.0 * sq) + np.abs(t)) + key * ulp32(t)

            tol_lo, tol_hi = tol(lo), tol(hi)
        e_disc = K * EPS * (2.0 * np.abs(h) * s_h + a * s_c)
        real, noreal = disc > 4.0 * e_disc, disc < -4.0 * e_disc
        on_in, on_out = (c == 0.0) & (h < 0.0), (c == 0.0) & (h >= 0.0)
        hit_lo = real & (lo > tol_lo) & ~on_in & ~on_out
        hit_hi = real & (hi > tol_hi) & (lo <= 0.0) & ~on_out
        miss = (noreal | (real & (hi < -tol_hi) & (lo < -tol_lo))) & ~on_out
        t = np.where(hit_lo, lo, hi)
        t_tol = np.where(hit_lo, tol_lo, tol_hi)
        sure = hit_lo | hit_hi
        miss = miss | (sure & (t - t_tol >= T_MAX))           # surely beyond the limit
        sure = sure & (t + t_tol < T_MAX)
        maybe = ~(sure | miss)
        # grazing bound around the double root, for pairs whose discriminant is not surely positive (module docstring)
        mid = -h / a
        tol_mid = np.sqrt(np.maximum(disc, 0.0) + 4.0 * e_disc) / a + K * EPS * (s_h / a + np.abs(mid)) + key * ulp32(mid)
        # the least t a MAYBE pair could return
        lb_maybe = np.where(real, np.where(lo + tol_lo > 0.0, lo - tol_lo, hi - tol_hi), mid - tol_mid)
        self.n_rays, self.n = o.shape[0], g.shape[0]
        self.a, self.h, self.c, self.disc, self.e_disc, self.real = a, h, c, disc, e_disc, real
        self.lo, self.hi, self.tol_lo, self.tol_hi, self.mid, self.tol_mid = lo, hi, tol_lo, tol_hi, mid, tol_mid
        self.t, self.tol, self.sure, self.miss, self.maybe, self.lb_maybe = t, t_tol, sure, miss, maybe, lb_maybe
        self.on_out = on_out

    def near_a_root(self, idx, t):
        """Per ray: is t within tol of a root of sphere idx[ray] (the weak check's t)?  -> (ok, ratio to the tolerance)."""
        r = np.arange(self.n_rays)
        t = np.asarray(t, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            e_lo = np.abs(t - self.lo[r, idx]) / self.tol_lo[r, idx]
            e_hi = np.abs(t - self.hi[r, idx]) / self.tol_hi[r, idx]
            e_mid = np.abs(t - self.mid[r, idx]) / self.tol_mid[r, idx]
        real = self.real[r, idx]
        ratio = np.where(real, np.fmin(e_lo, e_hi), e_mid)
        return ratio <= 1.0, ratio


class Rays:
    """The model's answer per ray."""

    def __init__(self, pairs, active=None):
        p = pairs
        sure, maybe = p.sure.copy(), p.maybe.copy()
        if active is not None:  # a ranking restricted to some spheres
            act = np.asarray(active, dtype=bool)[None, :]
            sure, maybe = sure & act, maybe & act
        t = np.where(sure, p.t, np.inf)
        self.idx = np.where(sure.any(1), t.argmin(1), -1)
        r = np.arange(p.n_rays)
        w = np.maximum(self.idx, 0)
        self.t = np.where(self.idx >= 0, p.t[r, w], np.inf)
        self.tol = np.where(self.idx >= 0, p.tol[r, w], 0.0)
        upper = np.where(self.idx >= 0, self.t + self.tol, np.inf)
        others = sure & (p.t - p.tol < upper[:, None])
        others[r, w] &= self.idx < 0
        self.decided = ~maybe.any(1) & ~others.any(1)
        self.possible = (sure & (p.t - p.tol < upper[:, None])) | (maybe & (p.lb_maybe < upper[:, None]))
        self.miss_possible = self.idx < 0
        self.pairs = pairs


def normal_at(o, d, g, radius, idx, t):
    """Float64 hit point and unit normal of sphere idx[ray] at t[ray], flipped by the reference's rule (dot(n, d) < 0, else
    negated; pathtrace.cu:163-166), and the per-component bound K eps (|o|_1 + |d|_1 t + |pos|_1 + |g|_1) / r + 4 eps."""
    o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3).astype(np.float64), np.asarray(d, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(t, dtype=np.float64)
    gc, r = g[idx].astype(np.float64), radius[idx].astype(np.float64)
    pos = o + d * t[:, None]
    n = (pos - gc) / r[:, None]
    n = n / np.sqrt((n * n).sum(-1))[:, None]
    flip = ~((n * d).sum(-1) < 0.0)
    n[flip] = -n[flip]
    bound = K * EPS * (np.abs(o).sum(-1) + np.abs(d).sum(-1) * np.abs(t) + np.abs(pos).sum(-1) + np.abs(gc).sum(-1)) / r + 4.0 * EPS
    return pos, n, bound


# ---- holding a list of answers (index or -1, t, optionally the normal) to the model ----------------------------------------
class Verdict:
    def __init__(self):
        self.failures, self.stats = [], {}

    def fail(self, what, rays, detail=""):
        rays = np.flatnonzero(rays)
        if len(rays):
            self.failures.append(f"{what}: {len(rays)} rays, first {rays[:6].tolist()} {detail}")

    def __bool__(self):
        return not self.failures

    def __str__(self):
        return "; ".join(self.failures) if self.failures else "ok"


def check_hits(model, idx, t, normal=None, o=None, d=None, g=None, radius=None, strong=True, t_exact=True):
    """idx [rays] (-1 = miss), t [rays], normal [rays][3] or None, against Rays `model`.  WEAK on all rays: the sphere is one of
    the possible winners (or a miss where a miss is possible), its t within tol of that sphere's model root, everything finite.
    STRONG on decided rays (strong=True): hit or miss and the sphere equal the model's, |t - t_model| <= tol, the normal within
    its bound of the model's normal at the answer's own t.  t_exact=False (the LAST shortcut: t is the truncated key) compares
    no t.  -> Verdict with stats {undecided, worst_t_ratio, worst_normal_ratio}."""
    v = Verdict()
    p = model.pairs
    idx, t = np.asarray(idx).astype(np.int64), np.asarray(t, dtype=np.float64)
    hit = idx >= 0
    r = np.arange(p.n_rays)
    w = np.maximum(idx, 0)
    v.fail("t not finite", hit & ~np.isfinite(t))
    v.fail("index out of range", idx >= p.n)
    w = np.minimum(w, p.n - 1)
    # weak
    v.fail("weak: miss where the model has a sure hit", ~hit & ~model.miss_possible)
    v.fail("weak: a sphere that cannot win", hit & ~model.possible[r, w])
    if t_exact:
        near, ratio = p.near_a_root(w, np.where(hit, t, 0.0))
        bad = hit & ~near
        v.fail("weak: t not within tol of a root of its sphere", bad, f"ratio {ratio[bad][:3]}" if bad.any() else "")
        v.fail("t <= 0", hit & ~(t > 0.0))
    dec = model.decided
    v.stats["undecided"] = float((~dec).mean())
    v.stats["worst_t_ratio"] = v.stats["worst_normal_ratio"] = 0.0
    if strong:
        v.fail("strong: hit/miss or sphere differs from the model", dec & (idx != model.idx),
               f"got {idx[dec & (idx != model.idx)][:6].tolist()} model {model.idx[dec & (idx != model.idx)][:6].tolist()}")
        both = dec & hit & (idx == model.idx)
        if t_exact and both.any():
            ratio = np.abs(t[both] - model.t[both]) / model.tol[both]
            v.stats["worst_t_ratio"] = float(ratio.max())
            bad = np.zeros_like(dec)
            bad[np.flatnonzero(both)[ratio > 1.0]] = True
            v.fail("strong: |t - t_model| > tol", bad, f"worst ratio {ratio.max():.3g}")
    if normal is not None and t_exact:
        sel = hit & np.isfinite(t) & ((dec & (idx == model.idx)) if strong else model.possible[r, w])
        if sel.any():
            _, n, bound = normal_at(o[sel], d[sel], g, radius, w[sel], t[sel])
            err = np.abs(np.asarray(normal, dtype=np.float64)[sel] - n).max(-1)
            ratio = err / bound
            if strong:
                v.stats["worst_normal_ratio"] = float(ratio.max())
            bad = np.zeros_like(dec)
            bad[np.flatnonzero(sel)[~(ratio <= 1.0)]] = True
            v.fail("normal beyond its bound of the model's at the answer's own t", bad, f"worst ratio {np.nanmax(ratio):.3g}")
    return v


def check_ray_list(o, d, spheres, ib, idx, t, active=None, strong=True, t_exact=True, chunk=8192):
    """check_hits for a long list of rays against a scene, the model built chunk by chunk.  active: the spheres ranked (a mask),
    None = all.  -> Verdict; .model_idx and .decided hold the model's answers."""
    o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3), np.asarray(d, dtype=np.float32).reshape(-1, 3)
    g, _, r2 = geometry(spheres)
    total = Verdict()
    total.stats = {"undecided": 0.0, "worst_t_ratio": 0.0, "worst_normal_ratio": 0.0}
    model_idx, decided = [], []
    for s in range(0, len(o), chunk):
        sl = slice(s, s + chunk)
        m = Rays(Pairs(o[sl], d[sl], g, r2, ib), active)
        v = check_hits(m, idx[sl], t[sl], strong=strong, t_exact=t_exact)
        total.failures += [f"rays from {s}: {f}" for f in v.failures]
        total.stats["undecided"] += v.stats["undecided"] * len(m.idx) / len(o)
        total.stats["worst_t_ratio"] = max(total.stats["worst_t_ratio"], v.stats["worst_t_ratio"])
        model_idx.append(m.idx)
        decided.append(m.decided)
    total.model_idx, total.decided = np.concatenate(model_idx), np.concatenate(decided)
    return total


def secondary_rays(case, count, seed, hemisphere=True):
    """count rays of the shape of every secondary ray (pathtrace.cu:178-180): origins are the model's hit points of the case's
    primary rays moved 0.05 along the normal and rounded to float32, directions random unit vectors -- in the hemisphere of that
    normal, where the cosine-weighted directions of the renderer lie (hemisphere=False: anywhere; half of those head straight back
    into the surface 0.05 behind the origin, and on a wall of radius 1e5 that hit at 0.05 / cos is inside its own tol of
    0.048 / cos whenever fl32(o - g) rounds the offset down, so a tenth of such a list is undecided by the model alone)."""
    m = case.model(0)
    o, d = case.rays()
    g, radius, _ = geometry(case.spheres)
    sel = m.decided & (m.idx >= 0)
    pos, n, _ = normal_at(o[sel], d[sel], g, radius, m.idx[sel], m.t[sel])
    origins = (pos + 0.05 * n).astype(np.float32)
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(count, 3))
    v /= np.sqrt((v * v).sum(-1))[:, None]
    pick = rng.integers(0, len(origins), count)
    if hemisphere:
        v = np.where(((v * n[pick]).sum(-1) < 0.0)[:, None], -v, v)
    return origins[pick], v.astype(np.float32)


def random_directions(count, seed):
    v = np.random.default_rng(seed).normal(size=(count, 3))
    return (v / np.sqrt((v * v).sum(-1))[:, None]).astype(np.float32)


# ---- frames -----------------------------------------------------------------------------------------------------------------
def unique_materials(spheres):
    """A copy with a colour and an emission no other sphere has: at 1 spp the albedo channels then name the first hit."""
    s = np.array(spheres, copy=True)
    i = np.arange(len(s), dtype=np.float32)
    s["color"][:, 0], s["color"][:, 1], s["color"][:, 2] = (i + 1.0) / 512.0, 0.5, 0.25
    s["emission"][:, 0], s["emission"][:, 1], s["emission"][:, 2] = (i + 1.0) / 1024.0, 0.125, 2.0  # the blue channel clamps to 1
    return s


def rays_of(basis, width, height, rows=None):
    """The primary directions of a frame without jitter (pathtrace.cu:221-229): d = lerp(lerp(B0, B1, col / w), lerp(B2, B3,
    col / w), 1 - row / h), interpolated in float64 and rounded once.  -> float32 [rows * width][3], row-major."""
    b = np.asarray(basis, dtype=np.float32).astype(np.float64).reshape(4, 3)
    rows = range(height) if rows is None else rows
    row, col = np.meshgrid(np.asarray(list(rows), dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    sy, u = (col / width).reshape(-1, 1), (1.0 - row / height).reshape(-1, 1)
    t0 = b[0] + sy * (b[1] - b[0])
    t1 = b[2] + sy * (b[3] - b[2])
    return (t0 + u * (t1 - t0)).astype(np.float32)


def fan(centre, right, up, half_width):
    """Basis of a fan of directions centre +- half_width right +- half_width up (twelve plain floats)."""
    c, r, u = (np.asarray(x, dtype=np.float64) for x in (centre, right, up))
    k = half_width
    return np.concatenate([c - k * r + k * u, c + k * r + k * u, c - k * r - k * u, c + k * r - k * u]).astype(np.float32)


def decode_frame(frame, spheres, max_bounces):
    """A 1 spp frame [pixels][14] of a scene with unique_materials -> (idx or -1, t, normal, Verdict of the frame's own rules):
    channels 6-8 carry the hit sphere's colour bits, 0-2 clamp(emission) (exactly so with one bounce; with more, later bounces
    only add non-negative light), 9 is t, 3-5 the normal, 10-13 are 0, a miss is all zeros."""
    v = Verdict()
    f = np.ascontiguousarray(frame, dtype=np.float32).reshape(-1, 14)
    v.fail("frame not finite", ~np.isfinite(f).all(1))
    bits = f.view(np.uint32)
    col = np.ascontiguousarray(spheres["color"], dtype=np.float32).view(np.uint32)
    same = (bits[:, None, 6:9] == col[None, :, :]).all(-1)
    idx = np.where(same.any(1), same.argmax(1), -1)
    blank = (bits == 0).all(1)
    v.fail("albedo names no sphere and the pixel is not blank", (idx < 0) & ~blank)
    v.fail("variance channels of a single sample not zero", (bits[:, 10:14] != 0).any(1))
    w = np.maximum(idx, 0)
    em = np.clip(np.ascontiguousarray(spheres["emission"], dtype=np.float32), 0.0, 1.0)[w]
    if max_bounces == 1:
        v.fail("colour is not clamp(emission) of the hit sphere", (idx >= 0) & (f[:, 0:3].view(np.uint32) != em.view(np.uint32)).any(1))
    else:
        v.fail("colour below clamp(emission) of the hit sphere", (idx >= 0) & ~(f[:, 0:3] >= em).all(1))
    return idx, f[:, 9].astype(np.float64), f[:, 3:6].astype(np.float64), v


class Case:
    def __init__(self, name, family, spheres, eye, basis, width, height, max_bounces=5, cap=None, strong=True):
        self.name, self.family, self.spheres = name, family, unique_materials(spheres)
        self.eye = np.asarray(eye, dtype=np.float32)
        self.basis = np.asarray(basis, dtype=np.float32).reshape(12)
        self.width, self.height, self.max_bounces, self.cap, self.strong = width, height, max_bounces, cap, strong
        self._model = {}

    @property
    def n(self):
        return len(self.spheres)

    def rays(self):
        d = rays_of(self.basis, self.width, self.height)
        return np.broadcast_to(self.eye, d.shape).copy(), d

    def model(self, ib):
        """Rays of the whole frame under a ranking of index width ib (computed once, shared, never changed)."""
        if ib not in self._model:
            o, d = self.rays()
            g, _, r2 = geometry(self.spheres)
            self._model[ib] = Rays(Pairs(o, d, g, r2, ib))
        return self._model[ib]

    def check(self, frame, ib):
        """Hold a whole 1 spp frame [height][width][14] to the model; -> Verdict (its stats carry the case's figures)."""
        idx, t, normal, v = decode_frame(frame, self.spheres, self.max_bounces)
        o, d = self.rays()
        g, radius, _ = geometry(self.spheres)
        m = self.model(ib)
        w = check_hits(m, idx, t, normal, o, d, g, radius, strong=self.strong)
        v.failures += w.failures
        v.stats = w.stats
        if self.cap is not None and v.stats["undecided"] > self.cap:
            v.failures.append(f"undecided share {v.stats['undecided']:.4f} above the case's cap {self.cap}")
        v.idx, v.t = idx, t
        return v


DEFAULT_EYE = (50.0, 52.0, 295.6)
LEFT_WALL_EYE = (1.0, 40.8, 81.6)  # exactly on the left wall sphere: off = (-1e5, 0, 0), |off|^2 = r2 = 1e10, c = 0
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def _sphere(pt, radius, pos):
    s = np.zeros(1, dtype=pt.SPHERE_DTYPE)
    s["radius"], s["pos"] = radius, pos
    return s


def zero_root_scene(pt, n):
    """Sphere A at the origin with r = 16 (the eye (16, 0, 0) lies exactly on it: 256 - 256), sphere B inside with r = 4, sphere
    C outside at (40, 0, 0) and sphere D beside the eye at (16, 40, 0), both r = 4, then far, small spheres nothing looks at, up to n."""
    parts = [_sphere(pt, 16.0, (0, 0, 0)), _sphere(pt, 4.0, (0, 0, 0)), _sphere(pt, 4.0, (40, 0, 0)), _sphere(pt, 4.0, (16, 40, 0))][:min(n, 4)]
    parts += [_sphere(pt, 1.0, (16.0, 1000.0 + 10.0 * i, 5000.0)) for i in range(n - len(parts))]
    return np.concatenate(parts)


def silhouette_fan(eye, centre, radius, half_width):
    """A fan centred on a direction from eye tangent to the sphere."""
    e, c = np.asarray(eye, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    to = c - e
    dist = np.sqrt((to * to).sum())
    f = to / dist
    side = np.cross(f, (0.0, 1.0, 0.0))
    side /= np.sqrt((side * side).sum())
    up = np.cross(side, f)
    sin = radius / dist
    d = f * np.sqrt(1.0 - sin * sin) + side * sin  # unit, tangent to the sphere
    right = side * np.sqrt(1.0 - sin * sin) - f * sin
    return fan(d, right, up, half_width)


def cases(pt):
    """Every case of tests/test_fast_rays_gpu.py ({name: Case}); tests/test_fast_model_host.py holds the oracle to the same."""
    out = []
    cornell = pt.scene_cornell()
    for (w, h) in ((64, 64), (41, 67)):  # 41 columns x 67 rows: neither is a multiple of the wave or the workgroup
        for mb in (5, 1, 8):
            out.append(Case(f"cornell_{w}x{h}_b{mb}", "cornell", cornell, DEFAULT_EYE, pt.camera_basis(width=w, height=h), w, h, mb, cap=0.02))
    inward = fan((-1, 0, 0), Z, Y, 0.3)
    for n in (2, 70):
        out.append(Case(f"zero_root_generic_n{n}", "zero_root", zero_root_scene(pt, n), (16, 0, 0), inward, 16, 16, 5, cap=0.0))
    out.append(Case("zero_root_cornell", "zero_root", cornell, LEFT_WALL_EYE, fan(X, Z, Y, 0.3), 32, 32, 5, cap=0.02))
    # the same eyes looking outward and along the tangent: the sphere under the eye is a MAYBE for every ray (no cap, weak only)
    for n in (4, 70):
        out.append(Case(f"outward_generic_n{n}", "on_surface_outward", zero_root_scene(pt, n), (16, 0, 0), fan(X, Z, Y, 0.3), 16, 16, 5, strong=False))
        out.append(Case(f"tangent_generic_n{n}", "on_surface_outward", zero_root_scene(pt, n), (16, 0, 0), fan(Y, Z, Y, 0.3), 16, 16, 5, strong=False))
    out.append(Case("outward_cornell", "on_surface_outward", cornell, LEFT_WALL_EYE, fan((-1, 0, 0), Z, Y, 0.3), 32, 32, 5, strong=False))
    out.append(Case("tangent_cornell", "on_surface_outward", cornell, LEFT_WALL_EYE, fan(Z, Z, Y, 0.3), 32, 32, 5, strong=False))
    s = cornell[7]
    out.append(Case("grazing_1e-2", "grazing", cornell, DEFAULT_EYE, silhouette_fan(DEFAULT_EYE, s["pos"], 16.5, 1e-2), 32, 32, 5, cap=0.05))
    out.append(Case("grazing_1e-4", "grazing", cornell, DEFAULT_EYE, silhouette_fan(DEFAULT_EYE, s["pos"], 16.5, 1e-4), 32, 32, 5))
    inside = (50.0, 40.0, 160.0)
    look = fan((0.0, -0.1, -1.0), X, Y, 0.5)
    for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 300):
        for walls in (False, True):
            if walls and n < 7:
                continue
            out.append(Case(f"random_n{n}_{'closed' if walls else 'open'}", "scene_sizes", pt.scene_random(n, seed=11, with_walls=walls), inside,
                            look, 32, 32, 2, cap=0.02))
    b64 = pt.camera_basis(width=64, height=64)
    shifted = np.array(cornell, copy=True)
    shifted["pos"] += np.float32(5000.0)
    out.append(Case("cornell_shifted_5000", "scale_position", shifted, np.asarray(DEFAULT_EYE, dtype=np.float32) + np.float32(5000.0), b64, 64, 64, 5, cap=0.02))
    small = np.array(cornell, copy=True)
    small["pos"] *= np.float32(1e-3)
    small["radius"] *= np.float32(1e-3)
    out.append(Case("cornell_scaled_1e-3", "scale_position", small, np.asarray(DEFAULT_EYE, dtype=np.float32) * np.float32(1e-3), b64, 64, 64, 5, cap=0.02))
    out.append(Case("cornell_basis_x50", "scale_position", cornell, DEFAULT_EYE, b64 * np.float32(50.0), 64, 64, 5, cap=0.02))
    out.append(Case("cornell_basis_x5e4", "scale_position", cornell, DEFAULT_EYE, b64 * np.float32(5e4), 64, 64, 5, cap=0.02))
    return {c.name: c for c in out}


def record(family, stats):
    """PT_FAST_RAYS_OUT=<file>: keep per case family the worst ratios and the largest undecided share seen (JSON)."""
    import json
    import os

    out = os.environ.get("PT_FAST_RAYS_OUT")
    if not out:
        return
    table = json.load(open(out)) if os.path.exists(out) else {}
    row = table.setdefault(family, {"K": K, "cases": 0, "worst_t_ratio": 0.0, "worst_normal_ratio": 0.0, "undecided_max": 0.0})
    row["cases"] += 1
    row["worst_t_ratio"] = max(row["worst_t_ratio"], stats["worst_t_ratio"])
    row["worst_normal_ratio"] = max(row["worst_normal_ratio"], stats["worst_normal_ratio"])
    row["undecided_max"] = max(row["undecided_max"], stats["undecided"])
    json.dump(table, open(out, "w"), indent=1, sort_keys=True)


def case_names():
    """The names of cases() without the library (test parametrisation happens before any fixture exists): the same code run
    on blank scene tables."""
    dtype = np.dtype([("radius", "<f4"), ("pos", "<f4", 3), ("emission", "<f4", 3), ("color", "<f4", 3)])

    class Blank:
        SPHERE_DTYPE = dtype
        scene_cornell = staticmethod(lambda: np.zeros(9, dtype=dtype))
        scene_random = staticmethod(lambda n, seed=0, with_walls=True: np.zeros(n, dtype=dtype))
        camera_basis = staticmethod(lambda width=1, height=1: np.zeros(12, dtype=np.float32))

    return list(cases(Blank))


# ---- float32 emulation of sphere_t and of the two rankings --------------------------------------------------------------------
def _fma(a, b, c):
    """fma of float32 arrays: the float64 product is exact, the sum is rounded to float64 and then once more to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_sphere_t(o, d, g, r2, fixed):
    """sphere_t of csrc/pt_fast.hip in float32 NumPy for rays [rays][3] against ONE sphere; square root and reciprocals are
    correctly rounded here (1 ulp on the GPU).  fixed=False is the root selection before the zero-root fix (one unsigned
    minimum of the two roots' bits), True the shipped one (the smallest denormal is subtracted from t_small first, so a zero
    gets the sign bit).  -> (t, disc) float32."""
    f = np.float32
    o, d = np.asarray(o, dtype=f).reshape(-1, 3), np.asarray(d, dtype=f).reshape(-1, 3)
    off = (o - np.asarray(g, dtype=f)[None, :]).astype(f)
    dot3 = lambda p, q: _fma(p[:, 0], q[:, 0], _fma(p[:, 1], q[:, 1], (p[:, 2] * q[:, 2]).astype(f)))
    with np.errstate(all="ignore"):
        a = dot3(d, d)
        inv_a = (f(1.0) / a).astype(f)
        h = dot3(d, off)
        c = (_fma(off[:, 2], off[:, 2], _fma(off[:, 1], off[:, 1], (off[:, 0] * off[:, 0]).astype(f))) - f(r2)).astype(f)
        disc = _fma(h, h, (-(a * c)).astype(f))
        s = np.sqrt(disc).astype(f)
        nq = (-np.copysign(s, h) - h).astype(f)
        t_big = (nq * inv_a).astype(f)
        t_small = (c * (f(1.0) / nq).astype(f)).astype(f)
        if fixed:
            t_small = (t_small - np.float32(2.0 ** -149)).astype(f)
    tb, ts = t_big.view(np.uint32), t_small.view(np.uint32)
    return np.where(tb < ts, tb, ts).astype(np.uint32).view(f), disc


def emulate_nearest(o, d, g, r2, fixed, keyed):
    """nearest<0> of csrc/pt_fast.hip over a scene: keyed=True ranks (bits(t) & ~imask) | i with one unsigned minimum per sphere
    and evaluates the winner again; False is the compare loop of scenes above 64 spheres.  -> (idx or -1, t float32)."""
    n_rays, n = np.asarray(o).reshape(-1, 3).shape[0], len(g)
    ts, discs = zip(*(emulate_sphere_t(o, d, g[i], r2[i], fixed) for i in range(n)))
    ts, discs = np.stack(ts, 1), np.stack(discs, 1)
    r = np.arange(n_rays)
    with np.errstate(invalid="ignore"):
        if keyed:
            imask = np.uint32((1 << index_bits(n)) - 1)
            keys = (ts.view(np.uint32) & ~imask) | np.arange(n, dtype=np.uint32)[None, :]
            best = keys.min(1)
            idx = (best & imask).astype(np.int64)
            t, disc = ts[r, idx], discs[r, idx]
            ok = (best < 0x7F800000) & (disc >= 0) & (t > 0) & (t < np.float32(T_MAX))
            return np.where(ok, idx, -1), t
        ok = (discs >= 0) & (ts > 0) & (ts < np.float32(T_MAX))
        tt = np.where(ok, ts, np.float32(np.inf))
        idx = tt.argmin(1)  # the first of equal t wins, as "t < best" in index order does
        return np.where(ok.any(1), idx, -1), tt[r, idx]
