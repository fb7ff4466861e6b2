"""Scenes, cameras and tiles of the primary-list tests (csrc/pt_primlist.h): shared by tests/test_primary_exclusion_host.py (the
NumPy model against the reference's intersection) and tests/test_primary_exclusion_gpu.py (the device's lists against the
model).  `pt` is the package; scenes and camera bases are host arithmetic of the library."""
import numpy as np

DEFAULT_EYE = (50.0, 52.0, 295.6)
WIDTHS = (192, 200, 320, 1024)
TILE_ROWS = 4


def camera(pt, sc, kind, seed, width, height):
    """The cameras of tools/primlist_soak.py: 0 the default view, 1 a hair outside a sphere's surface, 2 spheres behind the eye"""
    rng = np.random.default_rng(5150 + seed)
    k0 = 7 if len(sc) > 7 and sc["radius"][0] > 1000 else 0
    if kind == 0:
        eye, yaw = DEFAULT_EYE, -90.0
    elif kind == 1:
        j = k0 + int(rng.integers(0, len(sc) - k0))
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        eye = tuple(np.asarray(sc["pos"][j], dtype=np.float64) + v * float(sc["radius"][j]) * (1.0 + 10.0 ** rng.uniform(-4, -0.3)))
        yaw = float(rng.uniform(-130, -50))
    else:
        eye = tuple(rng.uniform([20, 20, -40], [80, 60, 60]))
        yaw = float(rng.choice([-90.0, 90.0]) + rng.uniform(-10, 10))
    return eye, pt.camera_basis(eye, yaw, float(rng.uniform(-25, 25)) if kind else 0.0, width, height)


def random_cases(pt, counts=(72, 300, 1000)):
    """[(name, spheres, eye, basis, width, height, row_begin, row_end)]: scene_random with and without walls, the three cameras,
    tiles of TILE_ROWS rows; every (scene, camera) pair at one of WIDTHS in rotation, so that every width meets every count"""
    out, turn = [], 0
    for n in counts:
        for walls in (True, False):
            sc = pt.scene_random(n, seed=n + (1 if walls else 0), with_walls=walls)
            for kind in (0, 1, 2):
                width = WIDTHS[turn % len(WIDTHS)]
                turn += 1
                eye, basis = camera(pt, sc, kind, n + kind, width, width)
                rb = width // 2 - TILE_ROWS // 2
                out.append((f"random{n}_{'walls' if walls else 'open'}_cam{kind}_w{width}", sc, eye, basis, width, width, rb, rb + TILE_ROWS))
    return out


def _small_spheres(pt, centres, radius):
    sc = pt.scene_random(len(centres), seed=1, with_walls=False).copy()
    sc["pos"] = np.asarray(centres, dtype=np.float32)
    sc["radius"] = np.float32(radius)
    return sc


def _pixel_dir(basis, width, height, row, col):
    B = np.asarray(basis, dtype=np.float64).reshape(4, 3)
    sx, sy = row / height, col / width
    top, bot = B[0] + (B[1] - B[0]) * sy, B[2] + (B[3] - B[2]) * sy
    return top + (bot - top) * (1.0 - sx)


def fallback_cases(pt):
    """The three fallbacks built on purpose, each with what it must hit (radius 0.5: the grid builder takes spheres from 2^-9 of
    the scene's extent, about 0.35 here, and these scenes must give a valid grid on the device):
    * six small spheres strung along ONE pixel's line of sight (plus a sprinkle elsewhere): that pixel's list is too long;
    * 300 small spheres inside ONE wave's 64-column strip at different depths: that wave's survivors exceed 256;
    * width 200: the waves that wrap from one row into the next span the image -- their cone is too wide."""
    width = height = 320
    eye = DEFAULT_EYE
    basis = pt.camera_basis(eye, -90.0, 0.0, width, height)
    rb = height // 2 - 2
    rng = np.random.default_rng(77)
    d = _pixel_dir(basis, width, height, rb + 1, 100)
    d /= np.linalg.norm(d)
    string = [np.asarray(eye) + d * t for t in (60.0, 75.0, 90.0, 105.0, 120.0, 135.0)]
    others = [np.asarray(eye) + _pixel_dir(basis, width, height, rb + rng.uniform(0, 4), c) / np.linalg.norm(_pixel_dir(basis, width, height, rb, c)) * rng.uniform(80, 200)
              for c in rng.uniform(0, 320, 40)]
    out = [("six_on_a_line", _small_spheres(pt, string + others, 0.5), eye, basis, width, height, rb, rb + 4, ("pixel", 1 * width + 100))]
    centres = []
    for i in range(300):  # columns 64 .. 127 of row rb + 2: lanes 704 .. 767 of the tile, one wave
        di = _pixel_dir(basis, width, height, rb + 2, 64.5 + 63.0 * (i % 60) / 59.0)
        centres.append(np.asarray(eye) + di / np.linalg.norm(di) * (50.0 + 0.6 * i))
    out.append(("strip_of_300", _small_spheres(pt, centres, 0.5), eye, basis, width, height, rb, rb + 4, ("wave", (2 * width + 64) // 64)))
    basis200 = pt.camera_basis(eye, -90.0, 0.0, 200, 200)
    out.append(("width_200", pt.scene_random(300, seed=3, with_walls=False), eye, basis200, 200, 200, 98, 102, ("wrapping_waves", None)))
    return out
