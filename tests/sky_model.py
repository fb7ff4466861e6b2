"""The definition of the sky and the sun (EXACTNESS.md A.24; the SKY builds of csrc/pt_materials.hip are bit-identical to it) in
NumPy float32, one rounding per operation.  Test infrastructure.

Built by import from tests/lights_model.py (the light list, the draws of light j, the cone sample's frame), tests/materials_model.py
(the bounce of every kind, the primary rays, both generators) and tests/numpy_restatement.py (the search, the hit geometry, the
Welford updates).  With sky=None the frame is `lights_model.render_frame`'s bit for bit.  What is new: the radiance an escaping path
takes, the colour Welford of escaped samples, the sun as the last light of A.23's list and the flag "sun accounted for".

A sky is a dict: zenith, horizon, ground (three floats each) and, optionally, sun_dir (towards the sun, any length), sun_cos,
sun_radiance.  `constants` is what the host forms from it.

render_frame returns (frame, info): info holds lights_model's counters and arms and, per frame,
  escaped_primary  paths whose primary ray finds nothing
  escaped_later    paths that leave after a bounce
  up, ground       ... of both, by u.y >= 0 or not
  sun_sampled      sun samples formed (a DIFFUSE hit at a sampling bounce)
  sun_lit          ... whose shadow ray finds nothing: the colour gained
  sun_shadowed     ... with cosl > 0 whose shadow ray met a sphere
  sun_below        ... with cosl <= 0: no ray
  sun_suppressed   escapes inside the sun's cone with the flag standing: base alone
  sun_kept         escapes inside the cone without the flag: base + sun_radiance
  sun_kept_after_specular  ... of those, the ones whose previous hit was MIRROR, GLOSSY or GLASS
`wrong="double"` and `wrong="drop"` are deliberately WRONG models for the tests' own sensitivity check: the first ignores the flag
(the sun counted twice), the second drops the sun from every escape after a bounce, flagged or not."""
import numpy as np

import lights_model as LM
import materials_model as MM
from numpy_restatement import EYE, PI_F, _cross, _dot, _hit_geometry, _luminance, _normalize, _variance, _welford, f32, intersect_scene

DIFFUSE = MM.DIFFUSE
ONE, TWO, ZERO = MM.ONE, MM.TWO, f32(0.0)
COUNTERS = ("escaped_primary", "escaped_later", "up", "ground", "sun_sampled", "sun_lit", "sun_shadowed", "sun_below", "sun_suppressed",
            "sun_kept", "sun_kept_after_specular")


def _ortho(v):  # ortho_vector (getCosineWeightedNormal, :126-129)
    zero = np.zeros_like(v[0])
    pick = np.abs(v[0]) > np.abs(v[2])
    neg = lambda x: (-x).astype(f32)  # noqa: E731
    return [np.where(pick, neg(v[1]), zero), np.where(pick, v[0], neg(v[2])), np.where(pick, zero, v[1])]


def constants(sky):
    """What pt_renderer_set_sky forms on the host, each operation rounded once in float32: slope = zenith - horizon; with a sun
    (any sun_radiance component > 0) the unit sun_dir = v * (1 / sqrt(dot(v, v))), the cone's frame o1 = normalize(ortho(dir)),
    o2 = normalize(cross(dir, o1)) and vers = 1 - sun_cos."""
    vec = lambda name: [np.asarray(f32(x)) for x in ((0.0, 0.0, 0.0) if sky.get(name) is None else sky[name])]  # noqa: E731
    zenith, horizon, ground, rad = vec("zenith"), vec("horizon"), vec("ground"), vec("sun_radiance")
    c = {"horizon": horizon, "ground": ground, "slope": [(zenith[k] - horizon[k]).astype(f32) for k in range(3)], "sun_radiance": rad,
         "has_sun": bool(any(r > 0 for r in rad))}
    if c["has_sun"]:
        dirn = _normalize(vec("sun_dir"))
        o1 = _normalize(_ortho(dirn))
        o2 = _normalize(_cross(dirn, o1))
        cos = f32(sky["sun_cos"])
        c.update(sun_dir=dirn, o1=o1, o2=o2, sun_cos=cos, vers=f32(ONE - cos))
    return c


def base_radiance(c, u):
    """The gradient: horizon + slope * u.y where u.y >= 0, ground elsewhere (a NaN is not >= 0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        up = u[1] >= 0
        return [np.where(up, (c["horizon"][k] + (c["slope"][k] * u[1]).astype(f32)).astype(f32), c["ground"][k]).astype(f32) for k in range(3)], up


def in_sun(c, u):
    if not c["has_sun"]:
        return np.zeros(u[0].shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        return _dot(u, c["sun_dir"]) >= c["sun_cos"]


def sun_sample(c, nl, u0, u1, sincos):
    """A.23's cone sample around sun_dir with vers given and the frame the host formed: (l, cosl, factor)."""
    with np.errstate(invalid="ignore", over="ignore"):
        vers = c["vers"]
        h = (u1 * vers).astype(f32)
        cos_a = (ONE - h).astype(f32)
        sin_a = np.sqrt((h * (TWO - h).astype(f32)).astype(f32)).astype(f32)
        rx = ((u0 * TWO).astype(f32) * PI_F).astype(f32)
        sn, cs = sincos(rx)
        ca, sa = (cs * sin_a).astype(f32), (sn * sin_a).astype(f32)
        l = _normalize([(((ca * c["o1"][k]).astype(f32) + (sa * c["o2"][k]).astype(f32)).astype(f32) + (cos_a * c["sun_dir"][k]).astype(f32)).astype(f32)
                        for k in range(3)])
        cosl = _dot(l, nl)
        factor = (cosl * f32(TWO * vers)).astype(f32)
    return l, cosl, factor


def render_frame(width, height, spp, spheres, basis, sincos, sky=None, materials=None, light_sampling=False, eye=EYE, max_bounces=5, seed=0,
                 rng="xorwow", philox=None, frame=0, row_begin=0, row_end=None, state=None, wrong=None):
    """The frame of the materials kernel's SKY builds for rows [row_begin, row_end): ((rows, width, 14) float32, info).
    sky=None: lights_model's frame.  materials: one (kind, param) per sphere, or None = every sphere DIFFUSE."""
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
    draws = LM._XorwowDraws(ids, seed, state) if rng == "xorwow" else LM._PhiloxDraws(ids, seed, frame, philox)
    everyone = np.ones(shape, dtype=bool)
    emission = np.asarray([s["emission"] for s in spheres], dtype=f32).reshape(-1, 3)
    colour_of = np.asarray([s["color"] for s in spheres], dtype=f32).reshape(-1, 3)
    centres = np.asarray([s["pos"] for s in spheres], dtype=f32).reshape(-1, 3)
    radii = np.asarray([s["radius"] for s in spheres], dtype=f32)
    lights = LM.light_list(spheres) if light_sampling else []
    c = constants(sky) if sky is not None else None
    sun_light = bool(light_sampling and c is not None and c["has_sun"])  # the sun is the LAST light: j = len(lights)
    zero = np.zeros(shape, dtype=f32)
    L_color, L_normal, L_albedo = [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)]
    L_depth = zero.copy()
    var = [(np.zeros(shape, dtype=np.int32), zero.copy(), zero.copy()) for _ in range(4)]
    info = {a: 0 for a in MM.ARMS + LM.COUNTERS + COUNTERS}
    info.update(capped=0, capped_live=0, paths=shape[0] * shape[1] * spp, lights=list(lights), lit_per_light=[0] * len(lights))
    is_light = np.zeros(len(spheres), dtype=bool)
    is_light[LM.light_list(spheres)] = True

    for s_i in range(spp):
        draws.begin_sample(s_i)
        jitter = draws.jitter(everyone) if spp != 1 else None
        o, d = MM._primary(rows, width, height, basis, eye, jitter)
        color = [zero.copy() for _ in range(3)]
        mask = [np.ones(shape, dtype=f32) for _ in range(3)]
        alive = everyone.copy()
        marked = np.zeros(shape, dtype=np.uint64)  # bit i: sphere i (a light) was sampled at the previous hit
        sunned = np.zeros(shape, dtype=bool)       # the sun was sampled at the previous hit
        after_specular = np.zeros(shape, dtype=bool)
        after_glossy = np.zeros(shape, dtype=bool)
        for n in range(max_bounces):
            hit, th, index = intersect_scene(o, d, spheres)
            gone = alive & ~hit
            if c is not None:  # an escaping path takes the sky's radiance
                u = _normalize(d) if n == 0 else d  # a primary ray is not of unit length
                base, up = base_radiance(c, u)
                inside = gone & in_sun(c, u)
                flagged = sunned if wrong != "double" else np.zeros(shape, dtype=bool)
                takes_sun = inside & ~flagged
                if wrong == "drop" and n > 0:
                    takes_sun = np.zeros(shape, dtype=bool)
                info["escaped_primary" if n == 0 else "escaped_later"] += int(np.count_nonzero(gone))
                info["up"] += int(np.count_nonzero(gone & up))
                info["ground"] += int(np.count_nonzero(gone & ~up))
                info["sun_suppressed"] += int(np.count_nonzero(inside & sunned))
                info["sun_kept"] += int(np.count_nonzero(inside & ~sunned))
                info["sun_kept_after_specular"] += int(np.count_nonzero(inside & ~sunned & after_specular))
                with np.errstate(invalid="ignore", over="ignore"):
                    for k in range(3):
                        rad = np.where(takes_sun, (base[k] + c["sun_radiance"][k]).astype(f32), base[k]).astype(f32)
                        mr = (mask[k] * rad).astype(f32)
                        if n == 0:  # the bright-source hack of :171-172
                            mr = np.fmax(f32(0.0), np.fmin(mr, f32(1.0)))
                        color[k] = np.where(gone, (color[k] + mr).astype(f32), color[k])
            alive = alive & hit
            p, nl = _hit_geometry(o, d, th, index, spheres)
            nr = _normalize([(p[k] - centres[index][..., k]).astype(f32) for k in range(3)])
            with np.errstate(invalid="ignore"):
                front = _dot(nr, d) < 0
            em, col = emission[index], colour_of[index]
            accounted = ((marked >> index.astype(np.uint64)) & np.uint64(1)) != 0
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
            cd = MM.cosine_direction(nl, u_az, u_el, sincos)
            o_next, d_next, weighted, weight, arms, _ = MM.material_step(p, nl, nr, front, d, cd, u_az, kinds[index], params[index], invs[index],
                                                                         r0s[index])
            for k in range(3):
                mask[k] = np.where(alive & weighted, (mask[k] * weight).astype(f32), mask[k])
            for a in MM.ARMS:
                info[a] += int(np.count_nonzero(alive & arms[a]))
            # direct light: the flags fall at every hit; the last bounce does not sample
            marked = np.zeros(shape, dtype=np.uint64)
            sunned = np.zeros(shape, dtype=bool)
            diffuse = alive & (kinds[index] == DIFFUSE)
            if (lights or sun_light) and n < max_bounces - 1:
                for j, li in enumerate(lights):
                    u0, u1 = draws.light(n, j, alive)  # every path that hit something, whatever the kind
                    itself = diffuse & (index == li)
                    l, cosl, vers, outside = LM.cone_sample(o_next, nl, centres[li], radii[li], u0, u1, sincos)
                    formed = diffuse & ~itself & outside
                    with np.errstate(invalid="ignore"):
                        above = formed & (cosl > 0)
                    s_hit, _, s_index = intersect_scene(o_next, l, spheres)
                    lit = above & s_hit & (s_index == li)
                    with np.errstate(invalid="ignore", over="ignore"):
                        factor = (cosl * (TWO * vers).astype(f32)).astype(f32)
                        for k in range(3):
                            gain = ((mask[k] * emission[li][k]).astype(f32) * factor).astype(f32)
                            color[k] = np.where(lit, (color[k] + gain).astype(f32), color[k])
                    marked = np.where(formed, marked | np.uint64(1 << li), marked)
                    info["self"] += int(np.count_nonzero(itself))
                    info["inside"] += int(np.count_nonzero(diffuse & ~itself & ~outside))
                    info["sampled"] += int(np.count_nonzero(formed))
                    info["below"] += int(np.count_nonzero(formed & ~above))
                    info["lit"] += int(np.count_nonzero(lit))
                    info["lit_per_light"][j] += int(np.count_nonzero(lit))
                    info["shadowed"] += int(np.count_nonzero(above & ~lit))
                if sun_light:  # the last light: no `outside`, no `self` -- the sun is nowhere
                    u0, u1 = draws.light(n, len(lights), alive)
                    l, cosl, factor = sun_sample(c, nl, u0, u1, sincos)
                    with np.errstate(invalid="ignore"):
                        above = diffuse & (cosl > 0)
                    s_hit, _, _ = intersect_scene(o_next, l, spheres)
                    lit = above & ~s_hit  # lit iff the search finds nothing
                    with np.errstate(invalid="ignore", over="ignore"):
                        for k in range(3):
                            gain = ((mask[k] * c["sun_radiance"][k]).astype(f32) * factor).astype(f32)
                            color[k] = np.where(lit, (color[k] + gain).astype(f32), color[k])
                    sunned = diffuse.copy()
                    info["sun_sampled"] += int(np.count_nonzero(diffuse))
                    info["sun_below"] += int(np.count_nonzero(diffuse & ~above))
                    info["sun_lit"] += int(np.count_nonzero(lit))
                    info["sun_shadowed"] += int(np.count_nonzero(above & ~lit))
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
        # a path's colour stands still once it has escaped: one addition per sample, escaped or not (:159 / :198)
        for k in range(3):
            L_color[k] = (L_color[k] + color[k]).astype(f32)
        # the decision of A.24: with a sky EVERY sample updates the colour Welford; without one only those that never escaped (:200)
        var[0] = _welford(var[0], _luminance(color), everyone if c is not None else alive)

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
