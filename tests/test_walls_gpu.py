"""The secondary-bounce wall certificate of the reference-configuration builds (pt_walls.h, pt_intersect.h screen_walled,
EXACTNESS.md A.18): on walled scenes the headline kernel ranks only the wall each ray faces on each axis and certifies the one
behind it.  Bar: bit-exact with the oracle, on scenes built to make the certificate fail (tiny boxes, where the 0.05 push of
pathtrace.cu:178 leaves origins outside walls; walls almost tangent to the objects; grazing rays), on moved and scaled boxes,
and on every kind of scene the classifier must reject, which take the path that screens all nine spheres."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assert_bit_exact(img, ref, what):
    neq = np.ascontiguousarray(img, dtype=np.float32).view(np.uint32) != np.ascontiguousarray(ref, dtype=np.float32).view(np.uint32)
    assert not neq.any(), f"{what}: {neq.sum()} floats differ"


def _box(pt, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """The Cornell box with every coordinate and radius scaled by `scale` about the origin and then moved by `shift`; the
    camera follows.  Radii stay 1e5 * scale for the walls, so a small scale makes the walls only ~1e3 box sizes large."""
    s = pt.scene_cornell()
    s["pos"] = (s["pos"].astype(np.float64) * scale + np.array(shift)).astype(np.float32)
    s["radius"] = (s["radius"].astype(np.float64) * scale).astype(np.float32)
    eye = tuple(float(np.float32(e * scale + d)) for e, d in zip((50.0, 52.0, 295.6), shift))
    return s, eye


def _render_both(pt, oracle, sph, eye, size=32, spp=4, yaw=-90.0, pitch=0.0, what=""):
    basis = pt.camera_basis(eye, yaw, pitch, size, size)
    for mb in (5, 8):  # the two reference-configuration builds (REF5, REF8)
        for rng in (0, 1):
            ref = oracle.render(size, size, spp, spheres=sph, basis=basis, eye=eye, rng_mode=rng, max_bounces=mb)
            img, _ = pt.render_frame(size, size, spp, spheres=sph, basis=basis, eye=eye, rng_mode=rng, max_bounces=mb, variant=6)
            _assert_bit_exact(img, ref, f"{what} bounces={mb} rng={rng}")


@pytest.mark.parametrize("scale,shift", [(1.0, (0.0, 0.0, 0.0)), (1e-3, (0.0, 0.0, 0.0)), (2e-3, (7.0, -3.0, 11.0)),
                                         (0.25, (-400.0, 250.0, 1000.0)), (40.0, (0.0, 0.0, 0.0)), (1.0, (1e4, -2e4, 5e3))],
                         ids=["cornell", "tiny", "tiny-moved", "small-moved", "large", "far"])
def test_moved_and_scaled_boxes(pt, oracle, gpu, scale, shift):
    sph, eye = _box(pt, scale, shift)
    _render_both(pt, oracle, sph, eye, what=f"box x{scale} +{shift}")


def test_eyes_near_walls_and_in_corners(pt, oracle, gpu):
    """Eyes 1e-3 from a wall and in corners, looking along the walls: the first bounce leaves from points near two or three
    walls at once, and grazing secondary rays have |d[axis]| down to the generator's resolution."""
    sph = pt.scene_cornell()
    for eye, yaw, pitch in (((1.001, 40.0, 100.0), 0.0, 0.0), ((98.999, 0.001, 0.001), 135.0, 20.0), ((1.001, 81.599, 0.001), 45.0, -30.0),
                            ((50.0, 0.001, 300.0), -90.0, 0.0), ((50.0, 40.0, 599.999), -90.0, 0.0), ((1.05, 0.05, 0.05), 45.0, 35.0)):
        _render_both(pt, oracle, sph, eye, yaw=yaw, pitch=pitch, what=f"eye {eye}")


def test_objects_touching_walls(pt, oracle, gpu):
    """Objects that touch or cut a wall: origins pushed off them land within the push distance of the wall or outside it."""
    sph = pt.scene_cornell()
    sph["pos"][6] = (1.0 + 16.5 - 1e-3, 16.5, 47.0)  # tangent to the left wall from inside, 1e-3 off
    sph["pos"][7] = (73.0, 16.5 - 0.02, 78.0)      # cuts the floor by 0.02
    _render_both(pt, oracle, sph, (50.0, 52.0, 295.6), what="objects on walls")


def _broken(pt, how):
    s = pt.scene_cornell()
    if how == "missing":  # a wall replaced by a small sphere
        s["radius"][1], s["pos"][1] = 5.0, (60.0, 30.0, 60.0)
    elif how == "emitting":
        s["emission"][2] = (0.5, 0.5, 0.5)
    elif how == "tilted":  # the left wall's centre off the box along two axes
        s["pos"][0] = (1e5 + 1.0, 40.8 + 3e3, 81.6)
    elif how == "duplicated":  # two floors
        s["pos"][5], s["radius"][5] = s["pos"][4], s["radius"][4]
    elif how == "nested":  # a second, smaller left wall inside the first, on the same side
        s["pos"][1], s["radius"][1] = (9e4 + 5.0, 40.8, 81.6), 9e4
    elif how == "open":  # the back wall turned round: the box is not closed along z
        s["pos"][3] = (50.0, 40.8, 1e5 + 700.0)
    return s


@pytest.mark.parametrize("how", ["missing", "emitting", "tilted", "duplicated", "nested", "open"])
def test_scenes_without_the_structure(pt, oracle, gpu, how):
    _render_both(pt, oracle, _broken(pt, how), (50.0, 52.0, 295.6), what=how)
