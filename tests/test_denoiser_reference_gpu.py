"""The denoising kernels (pt_denoiser_*, csrc/pt_denoise.hip) and the patch scores (pt_patches_*) against what the REFERENCE'S OWN
CODE computed: tests/golden/ref_denoise_*.npz (denoise_cnn/model.py, train.py:test and load_data.py:get_score executed in place
on the CPU by oracle/ref_denoise/record.py).  Only tests/golden is read.  Per tensor the yardstick is e32, the reference's own
float32 error against its float64 run: |hip - ref| <= 8 e32[tensor] + 4 ulp(ref)."""
import numpy as np
import pytest

import denoise_half_model as HM
import denoise_reference_fixture as fx
import patches_model as pm
from test_patches_host import bound as score_bound

pytestmark = pytest.mark.gpu

HALF_MAX = 65504.0


@pytest.fixture(scope="module")
def data():
    return fx.load()


@pytest.fixture(scope="module")
def sd(pt):
    from cuda_pathtrace_amd import denoise_weights

    return fx.state_dict(denoise_weights)


@pytest.fixture(scope="module")
def sessions(pt, lab, gpu, sd):
    """get(which, w, h, precision, max_frames) -> a denoiser of the product ("pt") or the lab library, made once per module
    from one PTDN image of the weights."""
    from cuda_pathtrace_amd import denoise_weights

    blob, made = denoise_weights.to_bytes(sd), {}

    def get(which, w, h, precision="float32", max_frames=1):
        key = (which, w, h, precision, max_frames)
        if key not in made:
            made[key] = {"pt": pt, "lab": lab}[which].Denoiser(w, h, blob, max_frames=max_frames, precision=precision)
        return made[key]

    yield get
    for dn in made.values():
        dn.destroy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hwc(t):
    """A recorded [C][h][w] tensor as the GPU lays an activation out: [h][w][C]."""
    return np.ascontiguousarray(np.transpose(t, (1, 2, 0)))


@pytest.mark.parametrize("precision", ["float32", "half"])
def test_preprocess_is_test_under_torch_0_2_bit_for_bit(pt, lab, sessions, data, precision):
    """Every input: channels 3-13 the in-place step leaves in the frame (product and lab library) and the network's stored
    input equal the tensor train.py:test() left in place under the torch 0.2/0.3 reading of torch.max, bit for bit (the half
    session stores that input rounded once to fp16)."""
    for w, h in fx.SIZES:
        s = fx.tag(w, h)
        frame, want = data[f"{s}/input"], data[f"{s}/pre_v02"]
        dn = sessions("lab", w, h, precision)
        after = lab.denoise_frame(frame, None, denoiser=dn)
        x0 = dn.activation(0)
        assert np.array_equal(bits(after[..., 3:14]), bits(want[..., 3:14])), s
        stored = want if precision == "float32" else np.clip(want, -HALF_MAX, HALF_MAX).astype(np.float16).astype(np.float32)
        assert np.array_equal(bits(x0[..., :14]), bits(stored)) and not x0[..., 14:].any(), s
        product = pt.denoise_frame(frame, None, denoiser=sessions("pt", w, h, precision))
        assert np.array_equal(bits(product[..., 3:14]), bits(want[..., 3:14])), s
        assert np.array_equal(bits(product), bits(after)), s


def _head_before_the_clamp(lab, dn, data, s):
    """The head computes clamp((rgb_conv(rep0) + bias) * (0.00316f + x0[6:9]), 0, 1) and stores nothing before the clamp, so a
    wrong value that stays outside [0, 1] would show nowhere.  After a whole pass (rep0 is the pass's own), the albedo
    channels of the stored input are replaced, element by element, by a - 0.00316f with a = +-2^k chosen from the RECORDED
    rgb_conv so that rgb_conv * a lies in (1/4, 1/2]: inside the clamp whatever the sign or size of the head's value.  The
    head runs alone; its output divided by the multiplier m = fl32(0.00316f + fl32(a - 0.00316f)), formed here exactly as the
    kernel forms it, is the head's value up to the one rounding of the product (half a float32 step, inside the bound's
    4).  -> {"rgb_conv": (that value, recorded rgb_conv), "preclamp": (that value times the frame's own fl32(0.00316f +
    albedo), recorded argument of the clamp)}, float64 [h][w][3]; every output asserted strictly inside (0, 1)."""
    keps = np.float32(0.00316)
    ref = hwc(data[f"{s}/aligned/rgb_conv"]).astype(np.float64)
    k = np.clip(np.floor(-1.0 - np.log2(np.maximum(np.abs(ref), 2.0 ** -100))), -100, 100)
    a = (np.where(ref < 0, -1.0, 1.0) * 2.0 ** k).astype(np.float32)
    scaled = np.abs(ref) * np.abs(a.astype(np.float64))
    assert np.all((scaled > 0.25) & (scaled <= 0.5)), "a recorded head value is 0 or out of the range of the scaling"
    x0 = dn.activation(0)
    albedo = x0[..., 6:9].copy()
    x0[..., 6:9] = a - keps
    m = (keps + x0[..., 6:9]).astype(np.float32)  # (one float32 add, as the kernel's)
    dn.set_activation(0, x0)
    head = [i for i, (_, info) in enumerate(dn.convs()) if info["out0"] < 0]
    assert len(head) == 1
    h, w = ref.shape[:2]
    d_out = lab.DeviceBuffer(h * w * 12)
    try:
        dn.run_conv(head[0], d_out.ptr)
        out = d_out.download(np.float32, (h, w, 3))
    finally:
        d_out.free()
    assert np.all((out > 0) & (out < 1)), "the probe's output reached the clamp"
    value = out.astype(np.float64) / m.astype(np.float64)
    own = (keps + albedo).astype(np.float32).astype(np.float64)
    return {"rgb_conv": (value, ref), "preclamp": (value * own, hwc(data[f"{s}/aligned/preclamp"]))}


@pytest.mark.parametrize("w,h", fx.PER_MODULE)
def test_every_stored_tensor_within_eight_times_the_references_float32_error(lab, sessions, data, w, h, capsys):
    """fp32 session, one whole pass, then every convolution's output(s) read back through layers(), convs() and activation():
    the two outputs of conv1+res_conv against the recorded batch-normed branches, conv2 against the block's output, lat_6 and
    each backwards_* against the ReLU of the recorded convolution, each lateral against the recorded _upsample_add, the head
    against the recorded result -- and, because the head clamps before it stores, the head BEFORE the clamp through a
    second run of the head alone (_head_before_the_clamp).  Bound: 8 e32[tensor] + 4 ulp(ref), e32 = max |the reference's
    float32 run - its float64 run|.
    Measured on an MI355X (worst (|err| - 4 ulp) / e32 per size): DENOISER.md, "Pinned to the reference's code"."""
    s = fx.tag(w, h)
    dn = sessions("lab", w, h)
    after = lab.denoise_frame(data[f"{s}/input"], None, denoiser=dn)
    want, e32 = fx.hip_view(dict(fx.tensors(data, s, "aligned"))), fx.e32(data, s)
    layers, ratios, failed = dn.layers(), {}, []
    for name, info in dn.convs():
        outs = [("final", after[..., 0:3])] if info["out0"] < 0 else [(layers[i][0], dn.activation(i)) for i in (info["out0"], info["out1"]) if i >= 0]
        for lname, got in outs:
            ref, source = want.pop(lname)
            ref = hwc(ref).astype(np.float64)
            assert got.shape == ref.shape, (name, lname, got.shape, ref.shape)
            err = np.abs(got.astype(np.float64) - ref)
            over = float(np.maximum(err - fx.ULPS * fx.ulp32(ref), 0.0).max())
            ratios[lname] = over / e32[source] if over > 0 else 0.0
            if not np.all(err <= fx.gpu_bound(ref, e32[source])):
                failed.append((lname, float(err.max()), e32[source]))
    assert not want, f"not checked: {sorted(want)}"
    for lname, (got, ref) in _head_before_the_clamp(lab, dn, data, s).items():
        err = np.abs(got - ref)
        over = float(np.maximum(err - fx.ULPS * fx.ulp32(ref), 0.0).max())
        ratios[lname] = over / e32[lname] if over > 0 else 0.0
        if not np.all(err <= fx.gpu_bound(ref, e32[lname])):
            failed.append((lname, float(err.max()), e32[lname]))
    with capsys.disabled():
        print(f"\n{s} worst (|hip - ref| - 4 ulp) / e32 per tensor (bound 8):", " ".join(f"{k}={v:.2f}" for k, v in ratios.items()))
        print(f"{s} overall worst: {max(ratios.values()):.2f}")
    assert not failed, failed


@pytest.mark.parametrize("w,h", fx.SIZES)
def test_fp32_end_to_end_against_the_recorded_float64_rgb(pt, sessions, data, w, h, capsys):
    """The result against the reference's float64 result within 1e-4; where the recorded PRE-CLAMP value lies outside [0, 1]
    the output is exactly 0 or 1 (the recipe keeps such values further from the clamp than the per-tensor bound); in place
    and out of place give the same bits."""
    s = fx.tag(w, h)
    dn = sessions("pt", w, h)
    frame = data[f"{s}/input"]
    after = pt.denoise_frame(frame, None, denoiser=dn)
    untouched, rgb = pt.denoise_frame(frame, None, out_of_place=True, denoiser=dn)
    assert np.array_equal(bits(untouched), bits(frame)) and np.array_equal(bits(rgb), bits(after[..., 0:3]))
    ref, pre = hwc(data[f"{s}/aligned/final"]), hwc(data[f"{s}/aligned/preclamp"])
    err = float(np.abs(rgb.astype(np.float64) - ref).max())
    with capsys.disabled():
        print(f"\n{s}: max |hip - recorded float64| {err:.3e}, clamped {float(((pre < 0) | (pre > 1)).mean()):.3f}")
    assert err <= fx.E2E_BOUND
    assert np.all(rgb[pre < 0] == 0.0) and np.all(rgb[pre > 1] == 1.0)
    assert (pre < 0).any() or w * h == 1


@pytest.mark.parametrize("w,h", [(19, 13), (37, 29), (64, 48)])
def test_half_end_to_end_within_the_models_error_of_the_recording(pt, sessions, data, sd, w, h, capsys):
    """Half session: E = GPU - recorded float64 rgb against Em = rounding model - recorded rgb by the limits of
    tests/test_denoiser_half_gpu.py (denoise_half_model.limits: max |E| <= 3 max |Em| + 1e-4, rms(E) <= 2 rms(Em) + 1e-5)."""
    s = fx.tag(w, h)
    frame = data[f"{s}/input"]
    ref = hwc(data[f"{s}/aligned/final"])
    model = HM.denoise(np.array(frame), sd, "fp16")
    lim_max, lim_rms = HM.limits(model, ref)
    after = pt.denoise_frame(frame, None, denoiser=sessions("pt", w, h, "half"))
    e_max, e_rms = HM.errors(after[..., 0:3], ref)
    with capsys.disabled():
        print(f"\n{s} half: GPU max {e_max:.3e} rms {e_rms:.3e} | limits max {lim_max:.3e} rms {lim_rms:.3e}")
    assert np.isfinite(after).all() and e_rms <= lim_rms and e_max <= lim_max


@pytest.mark.parametrize("precision", ["float32", "half"])
def test_a_group_of_three_gives_the_bits_of_the_single_calls(pt, sessions, data, precision):
    """The 19 x 13 input three times through enqueue_frames of a denoiser reserved for 2 frames (groups of 2 + 1)."""
    w, h = 19, 13
    frame = data[f"{fx.tag(w, h)}/input"]
    single = pt.denoise_frame(frame, None, denoiser=sessions("pt", w, h, precision))
    dn = sessions("pt", w, h, precision, max_frames=2)
    frames = np.stack([frame] * 3)
    d = pt.DeviceBuffer(frames.nbytes).upload(frames)
    try:
        dn.enqueue_frames(d.ptr, 3)
        pt.check(pt.lib.pt_device_synchronize())
        got = d.download(np.float32, frames.shape)
    finally:
        d.free()
    for f in range(3):
        assert np.array_equal(bits(got[f]), bits(single)), (precision, f)


def test_patch_scores_against_get_score(pt, gpu, data):
    """Patches.score on the fixture frames against load_data.py:get_score on the same patches, within the bound
    tests/test_patches_host.py derives for the model."""
    n = 0
    for w, h in fx.SIZES:
        s = fx.tag(w, h)
        frame = data[f"{s}/input"]
        pre = pm.preprocess(frame)
        for p in (8, 16):
            if f"{s}/score_P{p}" not in data:
                continue
            cs = [tuple(int(v) for v in c) for c in data[f"{s}/score_corners_P{p}"]]
            ps = pt.Patches(w, h, p, max_patches=len(cs))
            d = pt.DeviceBuffer(frame.nbytes).upload(frame)
            try:
                ps.run_prepare(d.ptr)
                ps.score(d.ptr, cs)
                got = ps.results(len(cs))
            finally:
                d.free()
                ps.destroy()
            for c, g, want in zip(cs, got, data[f"{s}/score_P{p}"]):
                assert abs(g["score"] - float(want)) <= score_bound(pre, c, p), (s, p, c, g["score"], float(want))
                n += 1
    assert n >= 20
