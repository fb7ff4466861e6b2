"""The scenes and cameras of the pixel-footprint tests (csrc/pt_footprint.h): the Cornell box with perturbed spheres and cameras
placed where the exclusion's criteria are closest to their limits.  Shared by tests/test_footprint_gpu.py (pictures against the
oracle), tests/test_primary_exclusion_host.py (the NumPy model against the reference's intersection) and
tests/test_primary_exclusion_gpu.py (the device's masks against the model).  `pt` is the package: the scene and the camera basis
are host arithmetic of the library, no device is needed."""
import numpy as np

BASE_SEEDS = tuple(range(16))
# Seeds of the same family beyond the first 16 on which a footprint radius x 0.3 is wrong in the MOST pixels (CPU search over seeds
# 16 .. 415 at 256 px, tests/test_primary_exclusion_host.py, search_seeds(): 44 of the 400 seeds notice it, these four in 85, 82,
# 72 and 67 pixels; EXACTNESS.md A.7): extra cases of the
# model's soundness and power tests and of the device's mask test.
EXTRA_SEEDS = (385, 195, 187, 246)


def case(pt, seed, size=None):
    """(spheres, eye, basis, size, row_begin, row_end, spp) of case `seed`; `size`: the same scene and camera at another
    (square) image size, whole frame."""
    rng = np.random.default_rng(91000 + seed)
    sc = pt.scene_cornell().copy()
    k = seed % 8
    scale = 1.0
    if k >= 1:
        sc["pos"][6:] += rng.normal(0, 8.0, size=(3, 3)).astype(np.float32)
        sc["radius"][6:8] *= rng.uniform(0.3, 2.5, 2).astype(np.float32)
    if k == 2:
        sc["pos"][:6] += rng.normal(0, 1.5, size=(6, 3)).astype(np.float32)
    if k == 3:
        sc["pos"][6] = (rng.uniform(0, 8), rng.uniform(0, 20), rng.uniform(20, 150))      # through a wall / the floor
    if k == 4:
        sc["pos"][7], sc["radius"][7] = sc["pos"][6], sc["radius"][6]                       # duplicate: first index wins
    if k == 5:
        sc["radius"][6] = rng.uniform(60, 400)                                              # eye inside a non-wall sphere
    if k == 6:
        scale = float(rng.choice([0.01, 100.0]))
        sc["pos"] *= np.float32(scale)
        sc["radius"] *= np.float32(scale)
    own_size = int(rng.choice([256, 320, 500, 512, 1024]))
    if k == 7:
        eye = tuple(rng.choice([[1.2, 40, 100], [98.9, 5, 20], [50, 81.3, 150], [2, 1, 2], [50, 40, 598]]) + rng.normal(0, 0.05, 3))
        yaw = float(rng.uniform(-180, 180))
    elif k == 1:
        eye = tuple((sc["pos"][6] + rng.normal(0, 1, 3) * (sc["radius"][6] * rng.choice([1.001, 1.02, 1.3]) + rng.choice([0.0, 5.0]))).astype(float))
        yaw = float(rng.uniform(-130, -50))
    else:
        eye = tuple(np.array(rng.uniform([10, 10, 120], [90, 70, 320])) * scale)
        yaw = float(rng.uniform(-130, -50))
    pitch = float(rng.uniform(-40, 40))
    if size is not None:
        return sc, eye, pt.camera_basis(eye, yaw, pitch, size, size), size, 0, size, 8
    basis = pt.camera_basis(eye, yaw, pitch, own_size, own_size)
    rb = 0 if own_size <= 512 else int(rng.integers(0, own_size - 128))
    re_ = own_size if own_size <= 512 else rb + 128
    return sc, eye, basis, own_size, rb, re_, int(rng.choice([8, 9, 16]))
