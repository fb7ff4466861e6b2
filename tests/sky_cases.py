"""Scenes, skies and closed forms shared by tests/test_sky_host.py and tests/test_sky_gpu.py.  Test infrastructure.

A sky is the dict tests/sky_model.py takes; `to_pt(pt, sky)` is the library's Sky of the same figures."""
import numpy as np

import materials_cases as MC

SPHERE_DTYPE = MC.SPHERE_DTYPE
EYE = MC.EYE
f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32

FLOOR_RADIUS, FLOOR_COLOUR = 1e4, 0.75


def _scene(rows):
    s = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for i, row in enumerate(rows):
        s[i] = tuple(row)
    return s


def floor():
    """One sphere of radius 1e4 whose top is y = 0, colour 0.75."""
    return (FLOOR_RADIUS, (50.0, -FLOOR_RADIUS, 81.6), (0.0, 0.0, 0.0), (FLOOR_COLOUR,) * 3)


def courtyard(box):
    """The floor and the box's two balls (spheres 6 and 7 of scene_cornell()) standing on it; no walls, no lamp.  Sphere 0 is the
    floor, 1 and 2 the balls."""
    return _scene([floor(), tuple(box[6]), tuple(box[7])])


COURTYARD_SMALLPT = [(MC.DIFFUSE, 0.0), (MC.MIRROR, 0.0), (MC.GLASS, 1.5)]  # SMALLPT_MATERIALS' two balls


def courtyard_three_lamps(box):
    """lights_cases.three_lamp_box's lamps moved into the courtyard: lights 3, 4, 5 of radii 1.5, 4 and 8, so the sun is light 3 of
    the list and, under Philox, draws from the block with counter word 3 = 2.  Lamp 4 reflects (colour 0.5)."""
    return _scene([floor(), tuple(box[6]), tuple(box[7]),
                   (1.5, (50.0, 65.1, 81.6), (400.0, 400.0, 400.0), (0.0, 0.0, 0.0)),
                   (4.0, (22.0, 30.0, 100.0), (30.0, 20.0, 10.0), (0.5, 0.5, 0.5)),
                   (8.0, (78.0, 60.0, 120.0), (4.0, 6.0, 8.0), (0.0, 0.0, 0.0))])


# ---- skies ---------------------------------------------------------------------------------------------------------------------------
GRADIENT = dict(zenith=(0.18, 0.36, 0.80), horizon=(0.80, 0.85, 0.90), ground=(0.25, 0.25, 0.25))  # CLEAR_SKY's
SUN_RADIANCE = (400.0, 380.0, 340.0)


def sky(sun_dir=None, sun_cos=None, sun_radiance=SUN_RADIANCE, **gradient):
    s = dict(GRADIENT)
    s.update(gradient)
    if sun_dir is not None:
        s.update(sun_dir=tuple(sun_dir), sun_cos=sun_cos, sun_radiance=tuple(sun_radiance))
    return s


SUNLESS = sky()
BLACK = dict(zenith=(0.0, 0.0, 0.0), horizon=(0.0, 0.0, 0.0), ground=(0.0, 0.0, 0.0))
# a wide sun's radiance is lower: 2 vers is a hundred times the small sun's
SUNS = {
    "small": sky((0.4, 0.8, 0.45), 0.999),                                # CLEAR_SKY: lit, shadowed by the balls, below on their far side
    "wide": sky((0.4, 0.8, 0.45), 0.9, (4.0, 3.8, 3.4)),                  # a cone of 26 degrees: bounces leave inside it -> suppressed
    "low": sky((-0.8, 0.25, 0.5), 0.9, (4.0, 3.8, 3.4)),                  # long shadows -> shadowed; below on half of each ball
    "in view": sky((0.05, 0.25, -1.0), 0.99, (40.0, 38.0, 34.0)),         # the disc inside the default view -> kept by primary rays
}


def to_pt(pt, s):
    return pt.Sky(s["zenith"], s["horizon"], s["ground"], s.get("sun_dir"), s.get("sun_cos"), s.get("sun_radiance"))


def counters(info):
    import sky_model as SM

    return {c: info[c] for c in SM.COUNTERS}


assert_same_bits = MC.assert_same_bits


# ---- closed form (a): every primary ray escapes ------------------------------------------------------------------------------------------
def behind_the_camera():
    """One small sphere behind the default camera (which looks along -z from z = 295.6): no primary ray meets it."""
    return _scene([(1.0, (50.0, 52.0, 400.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))])


ESCAPE_VIEWS = [(-90.0, 0.0), (-90.0, 14.0), (-60.0, -20.0)]  # (yaw, pitch): the horizon line; the sun's edge; mostly ground


def escape_closed_form(basis, size, s):
    """clamp(rad(normalize(d)), 0, 1) of every pixel's primary ray at 1 spp (no jitter), from the basis alone, float32, each operation
    rounded once: ((size, size, 3) colour, pixels above the horizon, pixels below it, pixels inside the sun's cone)."""
    B = np.asarray(basis, dtype=f32).reshape(4, 3)
    sx = (np.arange(size, dtype=f32) / f32(size))[:, None] * np.ones((1, size), dtype=f32)
    sy = np.ones((size, 1), dtype=f32) * (np.arange(size, dtype=f32) / f32(size))[None, :]
    lerp = lambda a, b, t: (a + (t * (b - a).astype(f32)).astype(f32)).astype(f32)  # noqa: E731
    one = np.ones((size, size), dtype=f32)
    d = [lerp(lerp(B[0, k] * one, B[1, k] * one, sy), lerp(B[2, k] * one, B[3, k] * one, sy), (f32(1.0) - sx).astype(f32)) for k in range(3)]
    dot = lambda a, b: (((a[0] * b[0]).astype(f32) + (a[1] * b[1]).astype(f32)).astype(f32) + (a[2] * b[2]).astype(f32)).astype(f32)  # noqa: E731
    inv = (f32(1.0) / np.sqrt(dot(d, d)).astype(f32)).astype(f32)
    u = [(d[k] * inv).astype(f32) for k in range(3)]
    up = u[1] >= 0
    sun = np.zeros((size, size), dtype=bool)
    if s.get("sun_radiance") is not None and any(x > 0 for x in s["sun_radiance"]):
        v = [f32(x) for x in s["sun_dir"]]
        vinv = f32(f32(1.0) / np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))))
        sd = [f32(x * vinv) for x in v]
        sun = dot(u, [sd[k] * one for k in range(3)]) >= f32(s["sun_cos"])
    out = np.zeros((size, size, 3), dtype=f32)
    for k in range(3):
        z, h, g = f32(s["zenith"][k]), f32(s["horizon"][k]), f32(s["ground"][k])
        rad = np.where(up, (h + (f32(z - h) * u[1]).astype(f32)).astype(f32), g).astype(f32)
        if sun.any():
            rad = np.where(sun, (rad + f32(s["sun_radiance"][k])).astype(f32), rad)
        out[..., k] = np.fmax(f32(0.0), np.fmin(rad, f32(1.0)))
    return out, int(np.count_nonzero(up)), int(np.count_nonzero(~up)), int(np.count_nonzero(sun))


def assert_escape_frame(img, basis, size, s, what):
    want, n_up, n_down, n_sun = escape_closed_form(basis, size, s)
    assert np.array_equal(img[..., :3].view(np.uint32), want.view(np.uint32)), f"{what}: colour differs from the closed form"
    assert not img[..., 3:].any(), f"{what}: a feature or a variance of a sky pixel is not zero"
    return n_up, n_down, n_sun


# ---- closed form (b): the furnace ---------------------------------------------------------------------------------------------------------
FURNACE_SKY = dict(zenith=(0.5, 0.5, 0.5), horizon=(0.5, 0.5, 0.5), ground=(0.5, 0.5, 0.5))


def furnace_ball():
    """One DIFFUSE sphere of colour 0.5 seen from outside (radius 30, 95.6 in front of the default camera)."""
    return _scene([(30.0, (50.0, 52.0, 200.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))])


def assert_furnace_frame(img, what, least=100):
    """A cosine bounce off a convex sphere always escapes, into a sky of 0.5 whichever way it goes: every sample that hits the ball is
    0.5 * 0.5 exactly.  The pixels whose four samples all hit it (albedo exactly 0.5: a miss contributes 0) hold colour 0.25 and
    colour variance 0, exactly."""
    whole = np.all(img[..., 6:9] == f32(0.5), axis=-1)
    assert np.count_nonzero(whole) >= least, (what, int(np.count_nonzero(whole)))
    assert np.all(img[whole][:, :3] == f32(0.25)) and np.all(img[whole][:, 10] == 0), what
    return int(np.count_nonzero(whole))


# ---- closed form (c): the sun on a floor --------------------------------------------------------------------------------------------------
SUN_FLOOR_EYE, SUN_FLOOR_YAW, SUN_FLOOR_PITCH = (50.0, 5.0, 150.0), -90.0, -89.0  # lights_cases.FLOOR_*: 5 above the floor, looking down
SUN_FLOOR_L, SUN_FLOOR_COS = 64.0, 0.999
SUN_FLOOR_SKY = dict(BLACK, sun_dir=(0.0, 1.0, 0.0), sun_cos=SUN_FLOOR_COS, sun_radiance=(SUN_FLOOR_L,) * 3)
# Float32 roundings between the definition's real-number value and the pixel, each at most one unit roundoff of a quantity no larger
# than the scale albedo * L * 2 vers (cosl <= 1): the hit point 2 per component and the normal's difference, normalisation and flip 6
# (nl: 8); the sample l = normalize((a + b) + c): cos_a, sin_a 4, the products and sums 4 per component, the normalisation 6 (l: 14);
# cosl = dot(l, nl) 5; the gain (mask * L) * (cosl * (2 vers)) 3; the float64 side reads a hit point the depth channel's rounding moved
# by one more.  31, taken as 32.  vers = 1 - 0.999f is exact in float32 (Sterbenz), doubling it too, the host's frame around (0, 1, 0)
# is exact, colour = 0 + gain and the division by 1 spp are exact.
SUN_FLOOR_ROUNDINGS = 32


def floor_only():
    return _scene([floor()])


def sun_floor_closed_form(img, basis, size):
    """Floor only, 1 spp, max_bounces = 2, a black sky with the sun overhead, light sampling on: a floor pixel holds exactly one sun
    sample (bounce 1 leaves the convex floor into a black sky with the flag standing: it adds 0), so its colour is
    albedo * L * 2 vers * cosl with l within a = acos(sun_cos) of the sun: colour in albedo * L * 2 vers * [cos(theta + a), cos(max(theta - a, 0))],
    theta (between the floor's normal and the sun) and a in float64 from the pixel's ray and its depth channel.
    Returns (pixels covered, pixels inside, widest interval as a share of the scale)."""
    B = np.asarray(basis, dtype=f64).reshape(4, 3)
    eye = np.asarray(SUN_FLOOR_EYE, dtype=f32).astype(f64)
    fc = np.asarray(floor()[1], dtype=f32).astype(f64)
    albedo, L, cos_a = f64(f32(FLOOR_COLOUR)), f64(f32(SUN_FLOOR_L)), f64(f32(SUN_FLOOR_COS))
    a = np.arccos(cos_a)
    scale = albedo * L * 2.0 * (1.0 - cos_a)
    sun = np.asarray([0.0, 1.0, 0.0])
    covered = passed = 0
    widest = 0.0
    for row in range(size):
        for col in range(size):
            if img[row, col, 6] != f32(FLOOR_COLOUR) or not img[row, col, 9] > 0:
                continue  # the first hit is not the floor
            sx, sy = f64(f32(row) / f32(size)), f64(f32(col) / f32(size))
            top, bot = B[0] + sy * (B[1] - B[0]), B[2] + sy * (B[3] - B[2])
            d = top + (1.0 - sx) * (bot - top)
            p = eye + d * f64(img[row, col, 9])
            nl = (p - fc) / np.linalg.norm(p - fc)
            theta = np.arccos(np.clip(np.dot(nl, sun), -1.0, 1.0))
            lo, hi = scale * np.cos(theta + a), scale * np.cos(max(theta - a, 0.0))
            widest = max(widest, (hi - lo) / scale)
            slack = SUN_FLOOR_ROUNDINGS * U
            lo, hi = lo * (1.0 - slack) - slack * scale, hi * (1.0 + slack) + slack * scale
            covered += 1
            passed += all(lo <= f64(img[row, col, k]) <= hi for k in range(3))
    return covered, passed, widest
