"""The definition of direct light sampling (EXACTNESS.md A.23; the LIGHTS build of csrc/pt_materials.hip is bit-identical to it) in
NumPy float32, one rounding per operation.  Test infrastructure.

Built by import from tests/materials_model.py (the bounce of every kind, the primary rays, both generators) and
tests/numpy_restatement.py (the search, the hit geometry, the Welford updates): with the option off, with no light in the scene
or with max_bounces = 1 the frame is `materials_model.render_frame`'s bit for bit (tests/test_lights_host.py, the anchors).  What
is new is the light list, the two draws per light, the cone sample and its shadow ray, and the mask of lights already accounted
for.

render_frame returns (frame, info): info holds materials_model's arms and, per frame,
  sampled     samples formed (a DIFFUSE hit at a sampling bounce, the light neither the hit sphere nor around the point)
  lit         ... whose shadow ray's nearest hit is the light: the colour gained
  shadowed    ... with cosl > 0 whose shadow ray met something else first (or nothing)
  below       ... with cosl <= 0: no ray
  inside      lights skipped because the point is not outside them (!(d2 > r2)); not marked
  self        lights skipped because they are the hit sphere; not marked
  suppressed  hits on a light whose emission was left out (the previous hit had sampled it)
  kept        hits on a light at n > 0 whose emission was added (not marked: after a specular hit, inside, self, the last bounce)
  kept_after_specular  ... of those, the ones whose previous hit was MIRROR, GLOSSY or GLASS
  kept_after_glossy    ... of those, the ones whose previous hit was GLOSSY (no pdf in A.22: it never samples, so nothing is marked)
  lit_per_light        `lit` per light, in list order
`double_count=True` is a deliberately WRONG model for the tests' own sensitivity check: it ignores the mask."""
import numpy as np

import materials_model as MM
from numpy_restatement import EYE, PI_F, _cross, _dot, _hit_geometry, _luminance, _normalize, _variance, _welford, f32, intersect_scene, u32

DIFFUSE = MM.DIFFUSE
ONE, TWO = MM.ONE, MM.TWO
COUNTERS = ("sampled", "lit", "shadowed", "below", "inside", "self", "suppressed", "kept", "kept_after_specular", "kept_after_glossy")


def light_list(spheres):
    """The indices of the spheres with any emission component > 0, in sphere order: light j is lights[j]."""
    return [i for i, s in enumerate(spheres) if np.any(np.asarray(s["emission"], dtype=f32) > 0)]


class _XorwowDraws(MM._XorwowDraws):
    def light(self, n, j, where):
        return self.g.uniform(where), self.g.uniform(where)  # u0 first


class _PhiloxDraws(MM._PhiloxDraws):
    """Light j at bounce n: counter (pixel, sample, n, 1 + (j >> 1)), words 2 (j & 1) and 2 (j & 1) + 1.  The path's own blocks have
    word 3 = 0, so they are untouched."""

    def light(self, n, j, where):
        if (j & 1) == 0 or getattr(self, "_lat", None) != (self.sample, n, j >> 1):
            self._lblk = np.zeros(self.ids.shape + (4,), dtype=u32)
            for at in np.ndindex(self.ids.shape):
                self._lblk[at] = self.philox((int(self.ids[at]), self.sample, n, 1 + (j >> 1)), self.key)
            self._lat = (self.sample, n, j >> 1)
        w = 2 * (j & 1)
        return MM._uniform_from_u32(self._lblk[..., w]), MM._uniform_from_u32(self._lblk[..., w + 1])


def cone_sample(x, nl, centre, radius, u0, u1, sincos):
    """One sample of the cone a sphere light subtends at x (A.23, line by line): (l, cosl, vers, formed-but-for-self).
    vers = 1 - cos(a_max) as q / (1 + cmax): no cancellation for a small lamp."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sw = [(f32(centre[k]) - x[k]).astype(f32) for k in range(3)]
        d2 = _dot(sw, sw)
        r2 = f32(f32(radius) * f32(radius))
        outside = d2 > r2  # a NaN is not outside
        q = (r2 / d2).astype(f32)
        cmax = np.sqrt((ONE - q).astype(f32)).astype(f32)
        vers = (q / (ONE + cmax).astype(f32)).astype(f32)
        h = (u1 * vers).astype(f32)
        cos_a = (ONE - h).astype(f32)
        sin_a = np.sqrt((h * (TWO - h).astype(f32)).astype(f32)).astype(f32)
        # getCosineWeightedNormal's frame (:126-129) around sw
        zero = np.zeros_like(sw[0])
        dirn = _normalize(sw)
        pick = np.abs(dirn[0]) > np.abs(dirn[2])
        neg = lambda v: (-v).astype(f32)  # noqa: E731
        ortho = [np.where(pick, neg(dirn[1]), zero), np.where(pick, dirn[0], neg(dirn[2])), np.where(pick, zero, dirn[1])]
        o1 = _normalize(ortho)
        o2 = _normalize(_cross(dirn, o1))
        rx = ((u0 * TWO).astype(f32) * PI_F).astype(f32)
        sn, cs = sincos(rx)
        ca, sa = (cs * sin_a).astype(f32), (sn * sin_a).astype(f32)
        l = _normalize([(((ca * o1[k]).astype(f32) + (sa * o2[k]).astype(f32)).astype(f32) + (cos_a * dirn[k]).astype(f32)).astype(f32)
                        for k in range(3)])
        cosl = _dot(l, nl)
    return l, cosl, vers, outside


def render_frame(width, height, spp, spheres, basis, sincos, materials=None, light_sampling=True, eye=EYE, max_bounces=5, seed=0, rng="xorwow",
                 philox=None, frame=0, row_begin=0, row_end=None, state=None, double_count=False):
    """The frame of the materials kernel with direct light sampling for rows [row_begin, row_end): ((rows, width, 14) float32, info).
    materials: one (kind, param) per sphere, or None = every sphere DIFFUSE.  light_sampling=False: the materials kernel's frame."""
    row_end = height if row_end is None else row_end
    rows = np.arange(row_begin, row_end)
    shape = (len(rows), width)
    if materials is None:
        materials = [(DIFFUSE, 0.0)] * len(spheres)
    assert len(materials) == len(spheres)
    kinds = np.asarray([int(m[0]) for m in materials], dtype=np.int32)
    params = np.asarray([m[1] for m in materials], dtype=f32)
    consts = [MM.glass_constants(m[1]) if int(m[0]) == MM.GLASS else (f32(0.0), f32(0.0)) for m in materials]
    invs, r0s = np.asarray([c[0] for c in consts], dtype=f32), np.asarray([c[1] for c in consts], dtype=f32)
    ids = rows.astype(np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    draws = _XorwowDraws(ids, seed, state) if rng == "xorwow" else _PhiloxDraws(ids, seed, frame, philox)
    everyone = np.ones(shape, dtype=bool)
    emission = np.asarray([s["emission"] for s in spheres], dtype=f32)
    colour_of = np.asarray([s["color"] for s in spheres], dtype=f32)
    centres = np.asarray([s["pos"] for s in spheres], dtype=f32)
    radii = np.asarray([s["radius"] for s in spheres], dtype=f32)
    lights = light_list(spheres) if light_sampling else []
    zero = np.zeros(shape, dtype=f32)
    L_color, L_normal, L_albedo = [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)]
    L_depth = zero.copy()
    var = [(np.zeros(shape, dtype=np.int32), zero.copy(), zero.copy()) for _ in range(4)]
    info = {a: 0 for a in MM.ARMS + COUNTERS}
    info.update(capped=0, capped_live=0, paths=shape[0] * shape[1] * spp, lights=list(lights), lit_per_light=[0] * len(lights))
    is_light = np.zeros(len(spheres), dtype=bool)
    is_light[light_list(spheres)] = True

    for s_i in range(spp):
        draws.begin_sample(s_i)
        jitter = draws.jitter(everyone) if spp != 1 else None
        o, d = MM._primary(rows, width, height, basis, eye, jitter)
        color = [zero.copy() for _ in range(3)]
        mask = [np.ones(shape, dtype=f32) for _ in range(3)]
        alive = everyone.copy()
        marked = np.zeros(shape, dtype=np.uint64)  # bit i: sphere i (a light) was sampled at the previous hit
        after_specular = np.zeros(shape, dtype=bool)
        after_glossy = np.zeros(shape, dtype=bool)
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
            accounted = ((marked >> index.astype(np.uint64)) & np.uint64(1)) != 0
            if double_count:
                accounted = np.zeros(shape, dtype=bool)
            on_light = alive & is_light[index]
            info["suppressed"] += int(np.count_nonzero(on_light & accounted))
            if n > 0 and lights:
                info["kept"] += int(np.count_nonzero(on_light & ~accounted))
                info["kept_after_specular"] += int(np.count_nonzero(on_light & ~accounted & after_specular))
                info["kept_after_glossy"] += int(np.count_nonzero(on_light & ~accounted & after_glossy))
            for k in range(3):
                me = (mask[k] * em[..., k]).astype(f32)
                if n == 0:
                    me = np.fmax(f32(0.0), np.fmin(me, f32(1.0)))
                color[k] = np.where(alive & ~accounted, (color[k] + me).astype(f32), color[k])
                mask[k] = np.where(alive, (mask[k] * col[..., k]).astype(f32), mask[k])
            u_az, u_el = draws.bounce(n, alive)  # for every kind, used or not
            c = MM.cosine_direction(nl, u_az, u_el, sincos)
            o_next, d_next, weighted, weight, arms, _ = MM.material_step(p, nl, nr, front, d, c, u_az, kinds[index], params[index], invs[index],
                                                                         r0s[index])
            for k in range(3):
                mask[k] = np.where(alive & weighted, (mask[k] * weight).astype(f32), mask[k])
            for a in MM.ARMS:
                info[a] += int(np.count_nonzero(alive & arms[a]))
            # direct light: the last bounce does not sample (its light path would be one segment longer than the frame allows)
            marked = np.zeros(shape, dtype=np.uint64)
            diffuse = alive & (kinds[index] == DIFFUSE)
            if lights and n < max_bounces - 1:
                for j, li in enumerate(lights):
                    u0, u1 = draws.light(n, j, alive)  # every path that hit something, whatever the kind
                    itself = diffuse & (index == li)
                    l, cosl, vers, outside = cone_sample(o_next, nl, centres[li], radii[li], u0, u1, sincos)
                    formed = diffuse & ~itself & outside
                    with np.errstate(invalid="ignore"):
                        up = formed & (cosl > 0)
                    s_hit, _, s_index = intersect_scene(o_next, l, spheres)
                    lit = up & s_hit & (s_index == li)
                    with np.errstate(invalid="ignore", over="ignore"):
                        factor = (cosl * (TWO * vers).astype(f32)).astype(f32)
                        for k in range(3):
                            gain = ((mask[k] * emission[li][k]).astype(f32) * factor).astype(f32)
                            color[k] = np.where(lit, (color[k] + gain).astype(f32), color[k])
                    marked = np.where(formed, marked | np.uint64(1 << li), marked)
                    info["self"] += int(np.count_nonzero(itself))
                    info["inside"] += int(np.count_nonzero(diffuse & ~itself & ~outside))
                    info["sampled"] += int(np.count_nonzero(formed))
                    info["below"] += int(np.count_nonzero(formed & ~up))
                    info["lit"] += int(np.count_nonzero(lit))
                    info["lit_per_light"][j] += int(np.count_nonzero(lit))
                    info["shadowed"] += int(np.count_nonzero(up & ~lit))
            after_specular = alive & ~diffuse
            after_glossy = alive & (kinds[index] == MM.GLOSSY)
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
