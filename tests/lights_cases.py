"""Scenes and helpers shared by tests/test_lights_host.py and tests/test_lights_gpu.py.  Test infrastructure.

Every scene that starts from the reference's box takes it as an argument (oracle.scene_cornell() or pt.scene_cornell(): the same
nine spheres) and returns a changed copy; sphere 8 is the box's lamp."""
import numpy as np

import materials_cases as MC

SPHERE_DTYPE = MC.SPHERE_DTYPE
EYE = MC.EYE
LAMP = 8  # the box's lamp: radius 600 above the ceiling


def _with(box, rows):
    s = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for i, row in enumerate(rows):
        s[i] = row if isinstance(row, tuple) else tuple(box[row])
    return s


def small_lamp_box(box):
    """smallpt's "explicit" lamp: sphere 8 replaced by radius 1.5 at (50, 65.1, 81.6), emission 400, colour 0."""
    return _with(box, list(range(8)) + [(1.5, (50.0, 65.1, 81.6), (400.0, 400.0, 400.0), (0.0, 0.0, 0.0))])


def three_lamp_box(box):
    """Eleven spheres, lights 8, 9, 10 of radii 1.5, 4 and 8.  Lamp 9 reflects (colour 0.5): it is DIFFUSE, samples the other two and
    must skip itself.  Under Philox light 2 draws from the block with counter word 3 = 2."""
    return _with(box, list(range(8)) + [(1.5, (50.0, 65.1, 81.6), (400.0, 400.0, 400.0), (0.0, 0.0, 0.0)),
                                         (4.0, (22.0, 30.0, 100.0), (30.0, 20.0, 10.0), (0.5, 0.5, 0.5)),
                                         (8.0, (78.0, 60.0, 120.0), (4.0, 6.0, 8.0), (0.0, 0.0, 0.0))])


def medium_lamp_box(box):
    """A closed box with a lamp of radius 8 under the ceiling: the same-expectation test's scene."""
    return _with(box, list(range(8)) + [(8.0, (50.0, 68.0, 81.6), (12.0, 12.0, 12.0), (0.0, 0.0, 0.0))])


FLOOR_COLOUR, FLOOR_LE, FLOOR_LAMP_R, FLOOR_LAMP_C, FLOOR_RADIUS = 0.75, 64.0, 10.0, (50.0, 100.0, 150.0), 1e4
FLOOR_EYE, FLOOR_YAW, FLOOR_PITCH = (50.0, 5.0, 150.0), -90.0, -89.0  # 5 above the floor, under the lamp, looking down


def floor_and_lamp(floor_radius=FLOOR_RADIUS):
    """An open scene with no occluder: the floor (a sphere below y = 0, colour 0.75) and a lamp of radius 10 whose centre is 100 units
    above it; the camera of FLOOR_EYE sees the few units of floor under the lamp, where r / d = 0.1 and the angle to the lamp's
    centre stays below 3 degrees.
    Why not a smaller r / d: the reference's sphere test decides `det >= 0` in float32, det = b b - 4 a c with b b about 4 d^2, so
    det = 4 r^2 (1 - u1) of a shadow ray carries a noise of a few ulps of 4 d^2, and a sample with 1 - u1 < 3 * 2^-23 / (r / d)^2
    may miss its own lamp.  At r / d = 0.0025 that is one sample in seventeen; at 0.1 it is 4e-5 per sample."""
    return _with(None, [(floor_radius, (50.0, -floor_radius, 81.6), (0.0, 0.0, 0.0), (FLOOR_COLOUR,) * 3),
                        (FLOOR_LAMP_R, FLOOR_LAMP_C, (FLOOR_LE,) * 3, (0.0, 0.0, 0.0))])


FLOOR_ROUNDINGS = 64  # tests/test_lights_host.py says where they go


def floor_closed_form(img, basis, size):
    """The closed form of the floor-and-lamp scene at 1 spp and max_bounces = 2, held against a frame (the model's or the device's):
    for every pixel whose first hit is the floor, is the colour inside albedo * Le * 2 vers * [cos(theta + a), cos(max(theta - a, 0))],
    widened by FLOOR_ROUNDINGS float32 roundings?  theta, a, d and vers in float64 from the pixel's ray (the basis) and its depth
    channel.  Returns (pixels covered, pixels inside, widest interval as a share of the scale)."""
    f32, f64, u = np.float32, np.float64, 2.0 ** -24
    sph = floor_and_lamp()
    B = np.asarray(basis, dtype=f64).reshape(4, 3)
    eye, C, R = np.asarray(FLOOR_EYE, dtype=f32).astype(f64), np.asarray(FLOOR_LAMP_C, dtype=f32).astype(f64), f64(f32(FLOOR_LAMP_R))
    fc = np.asarray(sph[0]["pos"], dtype=f64)
    albedo, le = f64(f32(FLOOR_COLOUR)), f64(f32(FLOOR_LE))
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
            x = p + 0.05 * nl
            sw = C - x
            dist = np.linalg.norm(sw)
            theta = np.arccos(np.clip(np.dot(nl, sw) / dist, -1.0, 1.0))
            a = np.arcsin(R / dist)
            if theta + a >= np.pi / 2:
                continue  # part of the lamp is below the horizon: the lower bound would be "0 or more"
            q = (R / dist) ** 2
            scale = albedo * le * 2.0 * (q / (1.0 + np.sqrt(1.0 - q)))
            lo, hi = scale * np.cos(theta + a), scale * np.cos(max(theta - a, 0.0))
            widest = max(widest, (hi - lo) / scale)
            slack = FLOOR_ROUNDINGS * u
            lo, hi = lo * (1.0 - slack) - slack * scale, hi * (1.0 + slack) + slack * scale
            covered += 1
            passed += all(lo <= f64(img[row, col, k]) <= hi for k in range(3))
    return covered, passed, widest


def glass_around_the_eye():
    """A closed, unlit diffuse shell (radius 300, colour 0.75), the eye INSIDE a glass sphere (materials_cases.inside_glass_furnace's
    geometry: radius 30, the eye 20 off its centre; INSIDE_ETA) and a lamp of radius 60 ahead to the right.  The middle of the view is
    beyond the critical angle and reflects totally inside the glass; the rays at the frame's right edge leave it, and that is where
    the lamp is, seen through the glass.  Materials: GLASS_AROUND_THE_EYE_TABLE."""
    return _with(None, [(300.0, (50.0, 52.0, 200.0), (0.0, 0.0, 0.0), (0.75, 0.75, 0.75)),
                        (30.0, (70.0, 52.0, 295.6), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                        (60.0, (130.0, 52.0, 120.0), (8.0, 6.0, 4.0), (0.0, 0.0, 0.0))])


GLASS_AROUND_THE_EYE_TABLE = [(MC.DIFFUSE, 0.0), (MC.GLASS, MC.INSIDE_ETA), (MC.DIFFUSE, 0.0)]
GLOSSY_BALLS = [(MC.DIFFUSE, 0.0)] * 6 + [(MC.GLOSSY, 0.3), (MC.GLOSSY, 0.3), (MC.DIFFUSE, 0.0)]  # the box's two balls, both GLOSSY 0.3


def no_light_box(box):
    s = box.copy()
    s["emission"] = 0.0
    return s


def two_lamps_among_twelve(spheres):
    """pt.scene_random(12, seed, with_walls=True) with its last two spheres emitting: past PT_SCREEN_MAX_SPHERES, the many-sphere
    path of the search."""
    s = spheres.copy()
    s["emission"] = 0.0
    s["emission"][-1] = (20.0, 16.0, 12.0)
    s["emission"][-2] = (6.0, 9.0, 12.0)
    return s


def counters(info):
    import lights_model as LM

    return {c: info[c] for c in LM.COUNTERS}


assert_same_bits = MC.assert_same_bits
