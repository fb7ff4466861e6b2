"""spatial_kernel (csrc/pt_filter.hip) on the exact cases of tests/filter_spatial_exact_cases.py: the variance after the set-up,
read through the lab library's pt_debug_filter_state with no step, against closed forms to the bit -- windows clipped by every
edge and corner, windows across the workgroup borders, a closed normal stop -- and everywhere against the float32 model's bits
(the weights are exactly 0 or 1 and the kernel's two moment sums round operation by operation in the model's order); pixels at
or above the threshold; non-finite pixels; a non-finite neighbour frame in a batch."""
import numpy as np
import pytest

import filter_model as fm
import filter_spatial_exact_cases as sx
import filter_spatial_model as fsm
from filter_exact_cases import bits
from test_filter_spatial_exact_host import CASES, model_var

pytestmark = pytest.mark.gpu


def device_var(lab, c, frame=None, below="all", counts=None):
    """The state's var after the set-up and the estimate, and the whole state, from the lab library."""
    frame = c["frame"] if frame is None else frame
    h, w = frame.shape[:2]
    ff = lab.FeatureFilter(w, h, spatial_below=below, spatial_radius=c["radius"], **c["sigmas"])
    bufs = [lab.DeviceBuffer(frame.nbytes).upload(np.ascontiguousarray(frame))]
    if counts is not None:
        bufs.append(lab.DeviceBuffer(h * w * 4).upload(np.ascontiguousarray(counts, dtype=np.uint32)))
    try:
        state, _, _ = ff.state(bufs[0].ptr, 0 if counts is not None else sx.N, (), d_counts=bufs[1].ptr if counts is not None else None)
    finally:
        for b in bufs:
            b.free()
        ff.destroy()
    return state[..., 3], state


@pytest.mark.parametrize("kind,radius", CASES, ids=[f"{k}-R{r}" for k, r in CASES])
def test_the_kernel_gives_the_closed_form(lab, gpu, kind, radius):
    """var = fmax(var0, v) with v the closed form wherever it is exact (every pixel for R = 1, 2; R = 3: all but some corner
    windows), and the float32 model's bits at every pixel; ill passes through untouched."""
    c = sx.case(kind, radius)
    v, exact, _ = sx.closed_form(c)
    got, state = device_var(lab, c)
    want = np.fmax(c["var0"], v)
    diff = exact & (bits(got) != bits(want))
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5])
    model = model_var(c)
    diff = bits(got) != bits(model)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5])
    assert np.array_equal(bits(state[..., :3]), bits(fm.setup(c["frame"], samples=sx.N, dtype=np.float32)[0]))
    assert (got[exact] > c["var0"][exact]).any()


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_pixels_at_or_above_the_threshold_keep_the_set_up(lab, gpu, radius):
    """A count image of below - 1, below, below + 1: at and above, the plain set-up's bits; below, the closed form."""
    c = sx.case("open", radius)
    h, w = c["var0"].shape
    counts = np.random.default_rng(radius).choice(np.array([3, 4, 5], dtype=np.uint32), (h, w))
    v, exact, _ = sx.closed_form(c)
    got, _ = device_var(lab, c, below=4, counts=counts)
    plain, _ = device_var(lab, c, below=0, counts=counts)
    assert np.array_equal(bits(plain), bits(fm.setup(c["frame"], counts=counts, dtype=np.float32)[1]))
    keep = counts >= 4
    assert np.array_equal(bits(got[keep]), bits(plain[keep]))
    low = ~keep & exact
    assert np.array_equal(bits(got[low]), bits(np.fmax(plain, v)[low]))
    assert np.array_equal(bits(got), bits(model_var(c, below=4, counts=counts)))
    assert (got[~keep] > plain[~keep]).any()


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_non_finite_pixel_reaches_its_window_and_leaves_var_alone(lab, gpu, radius, value):
    """NaN or +inf colour at a corner, on two edges, beside the workgroup borders and at the last pixel: exactly the pixels with
    it as an in-frame tap keep the set-up's var (fmax drops the NaN estimate), of whatever class (a weight of 0 does not shield
    a tap); every other pixel keeps the clean frame's bits -- a tap outside the frame reads one of the pixel's own taps."""
    for kind in sx.KINDS:
        c = sx.case(kind, radius)
        clean, _ = device_var(lab, c)
        for where in sx.POISON_AT[radius]:
            frame, at = sx.poisoned(c, where, value)
            reach = np.isnan(sx.closed_form(c, poison=at)[0])
            got, _ = device_var(lab, c, frame=frame)
            bad = reach & (bits(got) != bits(c["var0"]))
            assert not bad.any(), (kind, where, np.argwhere(bad)[:5])
            bad = ~reach & (bits(got) != bits(clean))
            assert not bad.any(), (kind, where, np.argwhere(bad)[:5])


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_non_finite_frame_next_door_reaches_nothing(pt, gpu, radius):
    """A batch of three frames in one group, the middle one the exact case, its neighbours and the stride gaps all NaN: the
    pixel just outside the frame in memory -- the neighbour's first or last, or the gap -- is never a tap, so the middle
    frame's output has the bits of a single enqueue."""
    c = sx.case("open", radius)
    frame = c["frame"]
    h, w = frame.shape[:2]
    single = pt.filter_frame(frame, sx.N, spatial_below="all", spatial_radius=radius, **c["sigmas"])
    assert np.isfinite(single).all()
    fs = w * h * 14 + 29
    host = np.full((3, fs), np.nan, np.float32)
    host[1, :w * h * 14] = frame.ravel()
    ff = pt.FeatureFilter(w, h, max_frames=3, spatial_below="all", spatial_radius=radius, **c["sigmas"])
    d_frames = pt.DeviceBuffer(host.nbytes).upload(host)
    try:
        ff.run_frames(d_frames.ptr, 3, sx.N, frame_stride_floats=fs)
        out = d_frames.download(np.float32, host.shape)
    finally:
        d_frames.free()
        ff.destroy()
    assert np.array_equal(bits(out[1, :w * h * 14].reshape(h, w, 14)), bits(single))
    assert np.isnan(out[1, w * h * 14:]).all()
