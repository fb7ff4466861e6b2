"""The definition of the sphere materials (EXACTNESS.md A.22; csrc/pt_materials.hip is bit-identical to it) in NumPy float32, one
rounding per operation.  Test infrastructure.

Built from the helpers of tests/numpy_restatement.py by import -- the search, the hit geometry, the generator, the Welford
updates are the restatement's own -- so that with an all-diffuse table the frame is `numpy_restatement.render_frame`'s bit for
bit (tests/test_materials_host.py, the anchor).  What is new is everything after the two draws of a bounce, written from the
definition's lines, and the counter-based generator (`philox` = oracle.philox, `sincos` = the oracle's pto_sincos as in
tests/test_full_path_numpy.py).

render_frame returns (frame, info): info counts the bounces that took each arm and the paths that ended at the bounce cap
(`capped`; `capped_live`: those that still carried weight there)."""
import numpy as np

from numpy_restatement import (EYE, PI_F, PUSH_RAY_ORIGIN, Xorwow, _cross, _dot, _hit_geometry, _lerp, _luminance, _normalize, _variance,
                               _welford, f32, f64, intersect_scene, u32)

DIFFUSE, MIRROR, GLOSSY, GLASS = 0, 1, 2, 3
ARMS = ("diffuse", "mirror", "glossy", "glass_reflect_front", "glass_reflect_inside", "glass_refract_front", "glass_refract_inside", "tir")
ONE, TWO, HALF, QUARTER = f32(1.0), f32(2.0), f32(0.5), f32(0.25)


def glass_constants(eta):
    """(1 / eta, R0) as the host forms them, in float32."""
    eta = f32(eta)
    em, ep = f32(eta - ONE), f32(eta + ONE)
    return f32(ONE / eta), f32(f32(em * em) / f32(ep * ep))


def sincos_of(oracle):
    both = np.frompyfunc(oracle.sincos, 1, 2)

    def sincos(x):
        s, c = both(x)
        return s.astype(f32), c.astype(f32)

    return sincos


def _uniform_from_u32(x):  # curand_uniform (contract C5), as numpy_restatement.Xorwow.uniform forms it
    c = f32(2.3283064e-10)
    return ((x.astype(f32) * c).astype(f32) + (c / f32(2.0)).astype(f32)).astype(f32)


class _XorwowDraws:
    def __init__(self, ids, seed, state):
        self.g = state if state is not None else Xorwow(ids + np.uint64(seed))

    def begin_sample(self, s):
        pass

    def jitter(self, where):
        return self.g.uniform(where), self.g.uniform(where)

    def bounce(self, n, where):
        return self.g.uniform(where), self.g.uniform(where)  # first draw -> azimuth (contract C5)


class _PhiloxDraws:
    """Rng<PT_RNG_PHILOX> (csrc/pt_scene_lds.h): counter (pixel, sample, block, 0), key (seed lo, seed hi ^ frame); block 0 holds the
    jitter and bounce 0, block b > 0 bounces 2b - 1 and 2b.  Stateless: `where` plays no part."""

    def __init__(self, ids, seed, frame, philox):
        self.ids = ids.astype(np.uint64)
        self.key = (u32(seed & 0xFFFFFFFF), u32(((seed >> 32) & 0xFFFFFFFF) ^ frame))
        self.philox = philox

    def _block(self, b):
        out = np.zeros(self.ids.shape + (4,), dtype=u32)
        for at in np.ndindex(self.ids.shape):
            out[at] = self.philox((int(self.ids[at]), self.sample, b, 0), self.key)
        return out

    def begin_sample(self, s):
        self.sample = s
        self.blk = self._block(0)

    def jitter(self, where):
        return _uniform_from_u32(self.blk[..., 0]), _uniform_from_u32(self.blk[..., 1])

    def bounce(self, n, where):
        if n & 1:
            self.blk = self._block((n + 1) >> 1)
        second = n == 0 or ((n + 1) & 1) != 0
        return _uniform_from_u32(self.blk[..., 2 if second else 0]), _uniform_from_u32(self.blk[..., 3 if second else 1])


def _primary(rows, width, height, basis, eye, jitter):  # :221-229 for the pixels of rows [row_begin, row_end): sx = row / height
    B = np.asarray(basis, dtype=f32).reshape(4, 3)
    x = rows.astype(f32)[:, None] * np.ones((1, width), dtype=f32)
    y = np.ones((len(rows), 1), dtype=f32) * np.arange(width, dtype=f32)[None, :]
    if jitter is not None:
        x = (x + ((jitter[0] * ONE).astype(f32) - HALF).astype(f32)).astype(f32)
        y = (y + ((jitter[1] * ONE).astype(f32) - HALF).astype(f32)).astype(f32)
    sx = (x / f32(height)).astype(f32)
    sy = (y / f32(width)).astype(f32)
    b0, b1, b2, b3 = ([np.full_like(sx, B[j, k]) for k in range(3)] for j in range(4))
    d = _lerp(_lerp(b0, b1, sy), _lerp(b2, b3, sy), (ONE - sx).astype(f32))
    o = [np.full_like(sx, f32(eye[k])) for k in range(3)]
    return o, d


def cosine_direction(nl, u_az, u_el, sincos):
    """normalize(getCosineWeightedNormal(nl)) (:126-136, :180), the lines of numpy_restatement.render_frame."""
    zero = np.zeros_like(nl[0])
    dirn = _normalize(nl)
    with np.errstate(invalid="ignore"):
        pick = np.abs(dirn[0]) > np.abs(dirn[2])
    neg = lambda v: (-v).astype(f32)  # noqa: E731
    ortho = [np.where(pick, neg(dirn[1]), zero), np.where(pick, dirn[0], neg(dirn[2])), np.where(pick, zero, dirn[1])]
    o1 = _normalize(ortho)
    o2 = _normalize(_cross(dirn, o1))
    rx = ((u_az * TWO).astype(f32) * PI_F).astype(f32)
    ry = np.sqrt(u_el).astype(f32)
    with np.errstate(invalid="ignore"):
        oneminus = np.sqrt(f64(1.0) - (ry * ry).astype(f32).astype(f64)).astype(f32)
    sn, cs = sincos(rx)
    ca, sa = (cs * oneminus).astype(f32), (sn * oneminus).astype(f32)
    nd = [(((ca * o1[k]).astype(f32) + (sa * o2[k]).astype(f32)).astype(f32) + (ry * dirn[k]).astype(f32)).astype(f32) for k in range(3)]
    return _normalize(nd)


def material_step(p, nl, nr, front, d, c, u_az, kind, param, inv, r0):
    """Everything of a bounce after the draws, for every kind (EXACTNESS.md A.22): the next origin and direction, the weight on the
    mask (None where the definition has none) and which arm was taken.  c = the DIFFUSE direction."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        o_out = [(p[k] + (nl[k] * PUSH_RAY_ORIGIN).astype(f32)).astype(f32) for k in range(3)]
        o_in = [(p[k] - (nl[k] * PUSH_RAY_ORIGIN).astype(f32)).astype(f32) for k in range(3)]
        du = _normalize(d)
        ddn = _dot(nl, du)
        two = (TWO * ddn).astype(f32)
        m = _normalize([(du[k] - (nl[k] * two).astype(f32)).astype(f32) for k in range(3)])
        gl = _normalize([(m[k] + ((c[k] - m[k]).astype(f32) * param).astype(f32)).astype(f32) for k in range(3)])
        nnt = np.where(front, inv, param).astype(f32)
        k_ = (ONE - ((nnt * nnt).astype(f32) * (ONE - (ddn * ddn).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        tir = ~(k_ >= 0)
        s = np.sqrt(k_).astype(f32)
        inner = ((ddn * nnt).astype(f32) + s).astype(f32)
        td = _normalize([((du[k] * nnt).astype(f32) - (nl[k] * inner).astype(f32)).astype(f32) for k in range(3)])
        cx = np.where(front, (-ddn).astype(f32), _dot(td, nr)).astype(f32)
        c1 = (ONE - cx).astype(f32)
        c2 = (c1 * c1).astype(f32)
        c5 = ((c2 * c2).astype(f32) * c1).astype(f32)
        re = (r0 + ((ONE - r0).astype(f32) * c5).astype(f32)).astype(f32)
        pr = (QUARTER + (HALF * re).astype(f32)).astype(f32)
        reflect = u_az < pr
        wr = (re / pr).astype(f32)
        wt = ((ONE - re).astype(f32) / (ONE - pr).astype(f32)).astype(f32)
    glass = kind == GLASS
    decided = glass & ~tir
    through = decided & ~reflect
    weight = np.where(reflect, wr, wt).astype(f32)
    d_next = [np.where(kind == DIFFUSE, c[k], np.where(kind == GLOSSY, gl[k], np.where(through, td[k], m[k]))) for k in range(3)]
    o_next = [np.where(through, o_in[k], o_out[k]) for k in range(3)]
    arms = {
        "diffuse": kind == DIFFUSE, "mirror": kind == MIRROR, "glossy": kind == GLOSSY,
        "glass_reflect_front": decided & reflect & front, "glass_reflect_inside": decided & reflect & ~front,
        "glass_refract_front": through & front, "glass_refract_inside": through & ~front, "tir": glass & tir,
    }
    return o_next, d_next, decided, weight, arms, {"re": re, "td": td, "tir": tir, "ddn": ddn, "m": m}


def render_frame(width, height, spp, spheres, basis, sincos, materials, eye=EYE, max_bounces=5, seed=0, rng="xorwow", philox=None, frame=0,
                 row_begin=0, row_end=None, state=None):
    """The materials kernel's frame for rows [row_begin, row_end): ((rows, width, 14) float32, info).  materials: one (kind, param)
    per sphere.  rng: "xorwow" (state: the numpy_restatement.Xorwow a previous frame left in info["state"], or None = seeded) or
    "philox" (philox = oracle.philox, frame = the renderer's frame counter)."""
    row_end = height if row_end is None else row_end
    rows = np.arange(row_begin, row_end)
    shape = (len(rows), width)
    assert len(materials) == len(spheres)
    kinds = np.asarray([int(m[0]) for m in materials], dtype=np.int32)
    params = np.asarray([m[1] for m in materials], dtype=f32)
    consts = [glass_constants(m[1]) if int(m[0]) == GLASS else (f32(0.0), f32(0.0)) for m in materials]
    invs, r0s = np.asarray([c[0] for c in consts], dtype=f32), np.asarray([c[1] for c in consts], dtype=f32)
    ids = rows.astype(np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    draws = _XorwowDraws(ids, seed, state) if rng == "xorwow" else _PhiloxDraws(ids, seed, frame, philox)
    everyone = np.ones(shape, dtype=bool)
    emission = np.asarray([s["emission"] for s in spheres], dtype=f32)
    colour_of = np.asarray([s["color"] for s in spheres], dtype=f32)
    centres = np.asarray([s["pos"] for s in spheres], dtype=f32)
    zero = np.zeros(shape, dtype=f32)
    L_color, L_normal, L_albedo = [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)]
    L_depth = zero.copy()
    var = [(np.zeros(shape, dtype=np.int32), zero.copy(), zero.copy()) for _ in range(4)]
    info = {a: 0 for a in ARMS}
    # capped: paths that made every bounce up to the cap; capped_live: those of them whose mask was not yet zero, i.e. the paths
    # whose remaining light the cap cut off (in a closed scene every path is capped; a furnace wall of colour 0 ends its weight)
    info.update(capped=0, capped_live=0, paths=shape[0] * shape[1] * spp)

    for s_i in range(spp):
        draws.begin_sample(s_i)
        jitter = draws.jitter(everyone) if spp != 1 else None
        o, d = _primary(rows, width, height, basis, eye, jitter)
        color = [zero.copy() for _ in range(3)]
        mask = [np.ones(shape, dtype=f32) for _ in range(3)]
        alive = everyone.copy()
        for n in range(max_bounces):
            hit, th, index = intersect_scene(o, d, spheres)
            gone = alive & ~hit
            for k in range(3):
                L_color[k] = np.where(gone, (L_color[k] + color[k]).astype(f32), L_color[k])
            alive = alive & hit
            p, nl = _hit_geometry(o, d, th, index, spheres)
            nr = _normalize([(p[k] - centres[index][..., k]).astype(f32) for k in range(3)])
            with np.errstate(invalid="ignore"):
                front = _dot(nr, d) < 0
            em, col = emission[index], colour_of[index]
            for k in range(3):
                me = (mask[k] * em[..., k]).astype(f32)
                if n == 0:
                    me = np.fmax(f32(0.0), np.fmin(me, f32(1.0)))
                color[k] = np.where(alive, (color[k] + me).astype(f32), color[k])
                mask[k] = np.where(alive, (mask[k] * col[..., k]).astype(f32), mask[k])
            u_az, u_el = draws.bounce(n, alive)  # for every kind, used or not
            c = cosine_direction(nl, u_az, u_el, sincos)
            o_next, d_next, weighted, weight, arms, _ = material_step(p, nl, nr, front, d, c, u_az, kinds[index], params[index], invs[index],
                                                                      r0s[index])
            for k in range(3):
                mask[k] = np.where(alive & weighted, (mask[k] * weight).astype(f32), mask[k])
            for a in ARMS:
                info[a] += int(np.count_nonzero(alive & arms[a]))
            if n == 0:
                lum_n, lum_a = _luminance(nl), _luminance([col[..., k] for k in range(3)])
                for k in range(3):
                    L_normal[k] = np.where(alive, (L_normal[k] + nl[k]).astype(f32), L_normal[k])
                    L_albedo[k] = np.where(alive, (L_albedo[k] + col[..., k]).astype(f32), L_albedo[k])
                L_depth = np.where(alive, (L_depth + th).astype(f32), L_depth)
                var[1] = _welford(var[1], lum_n, alive)
                var[2] = _welford(var[2], lum_a, alive)
                var[3] = _welford(var[3], th, alive)
            o = [np.where(alive, o_next[k], o[k]) for k in range(3)]
            d = [np.where(alive, d_next[k], d[k]) for k in range(3)]
        info["capped"] += int(np.count_nonzero(alive))
        info["capped_live"] += int(np.count_nonzero(alive & ((mask[0] != 0) | (mask[1] != 0) | (mask[2] != 0))))
        for k in range(3):
            L_color[k] = np.where(alive, (L_color[k] + color[k]).astype(f32), L_color[k])
        var[0] = _welford(var[0], _luminance(color), alive)

    out = np.zeros(shape + (14,), dtype=f32)
    nf = f32(spp)
    for k in range(3):
        out[..., k] = (L_color[k] / nf).astype(f32)
        out[..., 3 + k] = (L_normal[k] / nf).astype(f32)
        out[..., 6 + k] = (L_albedo[k] / nf).astype(f32)
    out[..., 9] = (L_depth / nf).astype(f32)
    for f in range(4):
        out[..., 10 + f] = _variance(var[f])
    if rng == "xorwow":
        info["state"] = draws.g
    return out, info
