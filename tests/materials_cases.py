"""Scenes and helpers shared by tests/test_materials_host.py and tests/test_materials_gpu.py.  Test infrastructure."""
import numpy as np

import materials_model as MM

SPHERE_DTYPE = np.dtype([("radius", "<f4"), ("pos", "<f4", 3), ("emission", "<f4", 3), ("color", "<f4", 3)])
EYE = (50.0, 52.0, 295.6)
E = (0.5, 0.25, 0.125)  # the furnace's emission: dyadic, so sums of equal values and their mean are exact

DIFFUSE, MIRROR, GLOSSY, GLASS = MM.DIFFUSE, MM.MIRROR, MM.GLOSSY, MM.GLASS


def _scene(rows):
    s = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for i, (radius, pos, emission, color) in enumerate(rows):
        s[i] = (radius, pos, emission, color)
    return s


def furnace(inner):
    """One enclosing sphere (radius 300 around (50, 52, 200): the eye is inside) that emits E and reflects nothing, and `inner`."""
    return _scene([(300.0, (50.0, 52.0, 200.0), E, (0.0, 0.0, 0.0))] + list(inner))


def ball_furnace():
    """A white ball of radius 30 in view, 95.6 units in front of the eye; its material is the test's: sphere 1."""
    return furnace([(30.0, (50.0, 52.0, 200.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])


INSIDE_ETA = 1.6


def inside_glass_furnace():
    """The eye sits INSIDE a white sphere of radius 30, 20 units off its centre, the centre to the eye's side.  A ray that leaves
    the eye at angle alpha to the line through the centre meets the surface at sin(theta) = (20 / 30) sin(alpha), and a chord keeps
    that angle at every later meeting.  So total internal reflection needs 1 / eta < 2 / 3 (eta = 1.5 sits exactly on it and never
    reflects totally) and rays near the perpendicular: with INSIDE_ETA = 1.6 the view holds both, rays beyond the critical angle
    (sin(alpha) > 0.9375) and rays below it, which leave the sphere."""
    return furnace([(30.0, (70.0, 52.0, 295.6), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])


def smallpt(glossy=False):
    """SMALLPT_MATERIALS, or the same with sphere 6 GLOSSY 0.3."""
    m = [(DIFFUSE, 0.0)] * 6 + [(MIRROR, 0.0), (GLASS, 1.5), (DIFFUSE, 0.0)]
    if glossy:
        m[6] = (GLOSSY, 0.3)
    return m


def arms(info):
    return {a: info[a] for a in MM.ARMS}


def assert_same_bits(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint32)
    w = np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, f"{what}: shape {g.shape} against {w.shape}"
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} of {g.size} floats differ, first at (row, col, channel) {tuple(bad[0])}: got " \
                          f"{got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}; channels hit {sorted(set(bad[:, 2]))}"
