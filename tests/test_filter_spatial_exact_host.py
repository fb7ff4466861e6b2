"""The float32 model of the spatial variance estimate (tests/filter_spatial_model.py) against the closed forms of
tests/filter_spatial_exact_cases.py, on the CPU: what test_filter_spatial_exact_gpu.py asks of the kernel is asked of the model
first, and the cases are shown to cover what they claim to cover."""
import numpy as np
import pytest

import filter_model as fm
import filter_spatial_exact_cases as sx
import filter_spatial_model as fsm
from filter_exact_cases import bits

CASES = [(kind, radius) for kind in sx.KINDS for radius in (1, 2, 3)]


def model_var(c, frame=None, below=fsm.ALL, counts=None):
    frame = c["frame"] if frame is None else frame
    s = c["sigmas"]
    return fsm.setup(frame, samples=None if counts is not None else sx.N, counts=counts, below=below, radius=c["radius"], sigma_n=s["sigma_n"],
                     sigma_a=s["sigma_a"], sigma_z=s["sigma_z"], dtype=np.float32)[1]


@pytest.mark.parametrize("kind,radius", CASES, ids=[f"{k}-R{r}" for k, r in CASES])
def test_the_model_gives_the_closed_form(kind, radius):
    c = sx.case(kind, radius)
    v, exact, taps = sx.closed_form(c)
    h, w = v.shape
    s = c["sigmas"]
    ill, var0, dz, _ = fm.setup(c["frame"], samples=sx.N, dtype=np.float32)
    got, sw, _ = fsm.estimate(ill, c["frame"], dz, radius, s["sigma_n"], s["sigma_a"], s["sigma_z"])
    assert np.array_equal(sw, taps.astype(np.float32))  # every weight is exactly 0 or 1
    assert np.array_equal(bits(got[exact]), bits(v[exact])), np.argwhere(exact & (bits(got) != bits(v)))[:5]
    want = np.fmax(var0, v)
    assert np.array_equal(bits(model_var(c)[exact]), bits(want[exact]))
    ys, xs = np.mgrid[0:h, 0:w]
    seen = exact & (v > 0)
    R = radius
    inner_x, inner_y = (xs >= R) & (xs < w - R), (ys >= R) & (ys < h - R)
    if kind == "normal":  # every window holds another class, and the closed form still has its pixels
        assert (taps < (2 * R + 1) ** 2).all() and (taps >= 1).all() and seen.sum() >= 20
        return
    # coverage: exact pixels with a lit tap in every corner, on every edge, in the interior, and whose windows cross the
    # workgroup borders x = 31 | 32 and y = 7 | 8
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert seen[y, x], (y, x)
    for name, where in (("top", (ys < R) & inner_x), ("bottom", (ys >= h - R) & inner_x), ("left", (xs < R) & inner_y),
                        ("right", (xs >= w - R) & inner_y), ("interior", inner_x & inner_y),
                        ("x border", (xs >= 32 - R) & (xs < 32 + R) & inner_y), ("y border", (ys >= 8 - R) & (ys < 8 + R) & inner_x)):
        assert (seen & where).any(), name
    assert exact.all() == (radius < 3) and exact.mean() > 0.9
    assert (taps[inner_y & inner_x] == (2 * R + 1) ** 2).all() and taps[0, 0] == (R + 1) ** 2


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_pixels_at_or_above_the_threshold_keep_the_set_up(radius):
    c = sx.case("open", radius)
    h, w = c["var0"].shape
    counts = np.random.default_rng(radius).choice(np.array([3, 4, 5], dtype=np.uint32), (h, w))
    v, exact, _ = sx.closed_form(c)
    got = model_var(c, below=4, counts=counts)
    var0 = fm.setup(c["frame"], counts=counts, dtype=np.float32)[1]
    keep = counts >= 4
    assert np.array_equal(bits(got[keep]), bits(var0[keep]))
    assert np.array_equal(bits(got[~keep & exact]), bits(np.fmax(var0, v)[~keep & exact]))
    assert (got[~keep] > var0[~keep]).any()


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_non_finite_pixel_reaches_its_window_and_leaves_var_alone(radius, value):
    """NaN or +inf colour at one pixel: exactly the pixels with it as an in-frame tap lose their estimate and keep the set-up's
    var (fmax); every other pixel keeps the clean frame's bits.  Both kinds: a weight of 0 does not shield a tap."""
    for kind in sx.KINDS:
        c = sx.case(kind, radius)
        clean = model_var(c)
        for where in sx.POISON_AT[radius]:
            frame, at = sx.poisoned(c, where, value)
            v, _, _ = sx.closed_form(c, poison=at)
            reach = np.isnan(v)
            assert reach[at] and reach.sum() > 1
            got = model_var(c, frame=frame)
            assert np.array_equal(bits(got[reach]), bits(c["var0"][reach])), (kind, where)
            assert np.array_equal(bits(got[~reach]), bits(clean[~reach])), (kind, where)
            if kind == "open":  # (there the clean estimate did raise var inside the reach: the check above is not vacuous)
                assert (clean[reach] != c["var0"][reach]).any(), where
