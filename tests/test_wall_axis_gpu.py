"""The per-axis form of the secondary-bounce wall screen (pt_intersect.h screen_walled, EXACTNESS.md A.21): the wall behind a ray
takes the two offsets, squares and products it shares with the faced wall of its axis from that wall, which is only right when
the two centres agree BIT FOR BIT in the other two coordinates -- the classifier (pt_walls.h) declines every other scene.
Bar: bit-exact with the oracle on all 14 channels, both generators, on the 5-bounce build (variant 6), for boxes that keep the
equality, boxes that break it by one ulp on each axis in turn, eyes next to walls, and a box whose pairs agree with each other on
two coordinates but not on the third.  64 x 16 pixels at 8 spp: complete waves, every bounce."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 16, 8
EYE = (50.0, 52.0, 295.6)


def _wall_pairs(s):
    """Per axis the indices (minus wall, plus wall) of the reference scene: the walls are the spheres of radius 1e5, a wall's
    axis is the coordinate that carries the 1e5."""
    pairs = [[None, None] for _ in range(3)]
    for i in range(len(s)):
        if s["radius"][i] >= 1e4:
            k = int(np.argmax(np.abs(s["pos"][i])))
            pairs[k][1 if s["pos"][i][k] > 0 else 0] = i
    assert all(p[0] is not None and p[1] is not None for p in pairs), pairs
    return pairs


def _moved(pt, scale, shift):
    """Every coordinate through the same float64 expression and one rounding: coordinates that were the same float stay so."""
    s = pt.scene_cornell()
    s["pos"] = (s["pos"].astype(np.float64) * scale + np.array(shift)).astype(np.float32)
    s["radius"] = (s["radius"].astype(np.float64) * scale).astype(np.float32)
    eye = tuple(float(np.float32(e * scale + d)) for e, d in zip(EYE, shift))
    return s, eye


def _check(pt, oracle, sph, eye, what, yaw=-90.0, pitch=0.0):
    basis = pt.camera_basis(eye, yaw, pitch, W, H)
    d_scene, n = pt.upload_scene(sph)
    d_out = pt.DeviceBuffer(W * H * pt.CHANNELS * 4)
    try:
        for rng in (0, 1):
            ref = oracle.render(W, H, SPP, spheres=sph, basis=basis, eye=eye, rng_mode=rng, max_bounces=5)
            r = pt.Renderer(W, H, SPP, max_bounces=5, rng_mode=rng, variant=6)
            try:
                r.render(d_out.ptr, d_scene.ptr, n, basis, eye)
                assert r.kernel_info(n)["variant"] == 6, r.kernel_info(n)
                img = d_out.download(np.float32, (H, W, pt.CHANNELS))
            finally:
                r.destroy()
            neq = img.view(np.uint32) != np.ascontiguousarray(ref, dtype=np.float32).reshape(img.shape).view(np.uint32)
            assert not neq.any(), f"{what} rng={rng}: {neq.sum()} floats differ"
    finally:
        d_out.free()
        d_scene.free()


def test_reference_scene(pt, oracle, gpu):
    _check(pt, oracle, pt.scene_cornell(), EYE, "cornell")


def test_box_moved_and_scaled_by_non_dyadic_factors(pt, oracle, gpu):
    sph, eye = _moved(pt, 0.37, (13.3, -7.1, 101.9))
    for lo, hi in _wall_pairs(pt.scene_cornell()):  # the construction keeps what the kernel shares
        same = sph["pos"][lo].view(np.uint32) == sph["pos"][hi].view(np.uint32)
        assert same.sum() == 2, (sph["pos"][lo], sph["pos"][hi])
    _check(pt, oracle, sph, eye, "box x0.37 moved")


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("which", [0, 1], ids=["first-shared", "second-shared"])
def test_one_ulp_between_the_walls_of_an_axis(pt, oracle, gpu, axis, which):
    """One shared coordinate of one wall of the pair moved by one ulp: the pair no longer has the equality, the scene must take
    the path that screens all nine spheres, and the frame stays exact."""
    sph, eye = _moved(pt, 0.37, (13.3, -7.1, 101.9))
    plus = _wall_pairs(pt.scene_cornell())[axis][1]
    j = [c for c in range(3) if c != axis][which]
    sph["pos"][plus][j] = np.nextafter(sph["pos"][plus][j], np.float32(np.inf))
    _check(pt, oracle, sph, eye, f"axis {axis}: coordinate {j} of wall {plus} one ulp up")


@pytest.mark.parametrize("eye,yaw,pitch", [((1.06, 40.0, 100.0), 0.0, 0.0), ((98.94, 0.06, 0.06), 135.0, 20.0)], ids=["near-wall", "corner"])
def test_eyes_near_a_wall_and_in_a_corner(pt, oracle, gpu, eye, yaw, pitch):
    _check(pt, oracle, pt.scene_cornell(), eye, f"eye {eye}", yaw=yaw, pitch=pitch)


def test_two_coordinates_shared_across_axes_and_one_not(pt, oracle, gpu):
    """Floor and ceiling moved half a unit along x, together: each pair keeps its own equality, y and z keep one value across the
    pairs that share them, x does not (50.5 for floor / ceiling, 50 for back / front)."""
    sph = pt.scene_cornell()
    lo, hi = _wall_pairs(sph)[1]
    sph["pos"][lo][0] = sph["pos"][hi][0] = np.float32(50.5)
    _check(pt, oracle, sph, EYE, "floor and ceiling at x = 50.5")
