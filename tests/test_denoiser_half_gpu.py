"""The denoiser's half-precision mode on the GPU (PT_DENOISE_F16: fp16 operands and storage, fp32 accumulation; DENOISER.md
"Half precision"): exact MFMA lane maps on integer data, the end-to-end error against the float64 network held to the error
of the rounding model (tests/denoise_half_model.py) on the same input, a per-layer rounding bound, saturation instead of
infinities, the frame channels the mode must not change, batches, determinism, workspace bytes and the CLI."""
import os
import subprocess

import numpy as np
import pytest
import torch

import denoise_half_model as HM
import denoise_restatement as R
from conftest import ROOT
from test_denoiser_gpu import _conv_ref64, _layer_outputs, _layer_ref, _pad_input_weight, _read_exr, _torch_names, bits, cornell

pytestmark = pytest.mark.gpu

HALF_MAX = 65504.0


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


@pytest.fixture(scope="module")
def sd(dw):
    return dw.random_state_dict(seed=1)


def _integer_state_dict(dw):
    """random_state_dict(integer=True) with batch norms whose folded affine is exactly (scale 1, integer shift), so that every
    exact layer output is an integer."""
    sdi = dw.random_state_dict(seed=5, integer=True)
    rs = np.random.default_rng(11)
    for k in list(sdi):
        if k.endswith(".running_mean"):
            base = k[: -len(".running_mean")]
            n = sdi[k].shape
            sdi[base + ".weight"] = np.ones(n, np.float32)
            sdi[base + ".bias"] = rs.integers(-3, 4, n).astype(np.float32)
            sdi[base + ".running_mean"] = np.zeros(n, np.float32)
            sdi[base + ".running_var"] = np.full(n, 1.0 - 1e-5, np.float32)
            s, t = dw.fold_bn(sdi, base)
            assert np.all(s == 1.0) and np.array_equal(t, sdi[base + ".bias"])
    return sdi


def test_half_mfma_lane_maps_are_exact_on_integer_data(pt, lab, gpu, dw):
    """One layer of each kind (3x3 stride 1 and 2, 1x1, fused conv1 + res_conv, split-K, lateral with upsample, head) and
    every half tile shape, on small-integer activations and the asymmetric integer weights.  The test first asserts that
    every exact (float64) output is an integer of magnitude <= 2048 -- so exactly representable in fp16, as every partial
    sum is in fp32 -- then demands bit equality.  At 129 x 129 every level is 2^a + 1 wide, so the align-corners bilinear
    weights are multiples of 1/4 and the upsample of a map of multiples of 16 is exact too."""
    sdi = _integer_state_dict(dw)
    rs = np.random.default_rng(9)
    picks = {256: ["block1.conv1+res_conv", "block1.conv2", "block2.conv1+res_conv", "lat_6", "block6.conv1+res_conv",
                   "block6.conv2", "backwards_10", "backwards_65"],
             1024: ["block3.conv1+res_conv", "block1.conv2"],
             129: ["lat_0", "lat_2", "lat_4", "backwards_21", "rgb_conv"]}
    seen_tiles, seen_split, seen_kinds = set(), False, set()
    for size, names in picks.items():
        dn = lab.Denoiser(size, size, sdi, precision="half")
        d_rgb = lab.DeviceBuffer(size * size * 12)
        try:
            assert dn.precision == "half"
            layers = dn.layers()
            convs = {n: (i, inf) for i, (n, inf) in enumerate(dn.convs())}
            for name in names:
                ci, info = convs[name]
                shape = layers[info["in"]][1]
                x = rs.choice(np.array([-1, 0, 0, 1], dtype=np.float32), size=shape)
                dn.set_activation(info["in"], x)
                assert np.array_equal(dn.activation(info["in"]), x)  # the lab exchange itself is exact on integers
                res = up = alb = None
                if info["res"] >= 0:
                    res = rs.integers(-3, 4, size=layers[info["res"]][1]).astype(np.float32)
                    dn.set_activation(info["res"], res)
                if info["up"] >= 0:
                    up = (16 * rs.integers(-3, 4, size=layers[info["up"]][1])).astype(np.float32)
                    dn.set_activation(info["up"], up)
                if info["epi"] == 2:
                    x0 = np.zeros(layers[0][1], np.float32)
                    x0[..., 6:9] = rs.choice(np.array([0.0, 0.0, 0.25], dtype=np.float32), size=x0[..., 6:9].shape)
                    dn.set_activation(0, x0)
                    alb = x0[..., 6:9]
                dn.run_conv(ci, d_rgb.ptr)
                got = [d_rgb.download(np.float32, (size, size, 3))] if info["out0"] < 0 else _layer_outputs(dn, ci, info)
                for k, (tname, bn) in enumerate(_torch_names(name)):
                    wgt = _pad_input_weight(sdi[tname + ".weight"], shape[2])
                    acc = _conv_ref64(x, wgt, info["stride"], info["ks"]) + sdi[tname + ".bias"].astype(np.float64)
                    if info["epi"] == 0:
                        v = np.maximum(acc, 0.0)
                        if bn:
                            v = v + sdi[bn + ".bias"].astype(np.float64)
                        if res is not None:
                            v = v + res
                    elif info["epi"] == 1:
                        u = torch.from_numpy(up.astype(np.float64)).permute(2, 0, 1).unsqueeze(0)
                        v = R.upsample(u, shape[:2])[0].permute(1, 2, 0).numpy() + np.maximum(acc, 0.0)
                    else:
                        v = acc
                    assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 2048, (name, float(np.abs(v).max()))
                    if info["epi"] == 2:  # the head is fp32: two correctly rounded fp32 operations on exact operands
                        ref = np.clip(v.astype(np.float32) * (np.float32(R.KEPS) + alb), np.float32(0), np.float32(1))
                        assert 0.05 < float(((ref > 0) & (ref < 1)).mean())
                    else:
                        ref = v.astype(np.float32)
                    g = got[k]
                    assert g.shape == ref.shape, name
                    bad = np.argwhere(bits(g) != bits(ref))
                    assert len(bad) == 0, f"{name}: {len(bad)} differ, first {bad[:3].tolist()} {g[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
                seen_tiles.add((info["bm"], info["bn"]))
                seen_split |= info["splits"] > 1
                seen_kinds.add((info["ks"], info["stride"], info["epi"]))
        finally:
            d_rgb.free()
            dn.destroy()
    assert seen_tiles == {(256, 32), (128, 64), (128, 128), (128, 32), (64, 64)} and seen_split, seen_tiles
    assert seen_kinds >= {(3, 1, 0), (3, 2, 0), (1, 1, 0), (1, 1, 1), (3, 1, 2)}, seen_kinds


_refs = {}


def _reference(pt, w, h, seed, sdk):
    """(float64 rgb, model rgb) of the rendered Cornell frame: both from the same input, computed once per case."""
    if (w, h, seed) not in _refs:
        frame = cornell(pt, w, h)
        _refs[(w, h, seed)] = (HM.denoise(frame, sdk, None), HM.denoise(frame, sdk, "fp16"))
    return _refs[(w, h, seed)]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("w,h", [(100, 75), (512, 512), (1024, 1024)])
def test_half_end_to_end_error_is_the_models(pt, gpu, dw, w, h, seed, capsys):
    """With E = GPU - float64 and Em = model - float64 on the same frame: rms(E) <= 2 rms(Em) + 1e-5 and max|E| <= 3 max|Em| +
    1e-4, in place and out of place; at least half of the compared outputs lie strictly inside (0, 1).  Kernel and model are
    two draws of the same rounding process (fp32 instead of float64 sums flip individual fp16 roundings); a bf16-sized error
    (3 x and more in rms) fails."""
    sdk = dw.random_state_dict(seed=seed)
    frame = cornell(pt, w, h)
    ref, model = _reference(pt, w, h, seed, sdk)
    m_max, m_rms = HM.errors(model, ref)
    inside = float(((ref > 0) & (ref < 1)).mean())
    dn = pt.Denoiser(w, h, sdk, precision="half")
    try:
        after = pt.denoise_frame(frame, None, denoiser=dn)
        untouched, rgb = pt.denoise_frame(frame, None, out_of_place=True, denoiser=dn)
    finally:
        dn.destroy()
    assert np.array_equal(bits(untouched), bits(frame))
    for what, got in (("in place", after[..., 0:3]), ("out of place", rgb)):
        assert np.isfinite(got).all()
        e_max, e_rms = HM.errors(got, ref)
        with capsys.disabled():
            print(f"\n{w}x{h} seed {seed} {what}: GPU max {e_max:.3e} rms {e_rms:.3e} | model max {m_max:.3e} rms {m_rms:.3e} | "
                  f"inside (0,1) {inside:.3f}")
        lim_max, lim_rms = HM.limits(model, ref)  # 3 max|Em| + 1e-4, 2 rms(Em) + 1e-5
        assert e_rms <= lim_rms, (what, e_rms, m_rms)
        assert e_max <= lim_max, (what, e_max, m_max)
    assert inside >= 0.5


def test_half_per_layer_rounding_within_the_bound(pt, lab, gpu, dw, sd, capsys):
    """Every layer, from the half input of that layer, against float64 on that same (already rounded) input and the rounded
    weights: |hip - ref| <= 4e-6 S + 4 ulp32(ref) + 1 ulp16(ref) -- the fp32 mode's bound plus the one rounding of the store
    (the head stores fp32: no ulp16 term).  Saturated elements are compared with +-65504.  At 256 x 256 and at 37 x 29 (every
    M ragged, maps down to 1 x 1), the same bound."""
    for w, h in ((256, 256), (37, 29)):
        _half_per_layer_rounding(pt, lab, dw, sd, capsys, w, h)


def _half_per_layer_rounding(pt, lab, dw, sd, capsys, w, h):
    frame = cornell(pt, w, h)
    sdh = {k: (np.clip(v, -HALF_MAX, HALF_MAX).astype(np.float16).astype(np.float32) if v.ndim == 4 else v) for k, v in sd.items()}
    dn = lab.Denoiser(w, h, sd, precision="half")
    worst = {}
    try:
        d_frame = lab.DeviceBuffer(frame.nbytes).upload(frame)
        d_rgb = lab.DeviceBuffer(w * h * 12)
        dn.denoise(d_frame.ptr, d_rgb.ptr)
        rgb = d_rgb.download(np.float32, (h, w, 3))
        layers = dn.layers()
        x0 = dn.activation(0)
        for ci, (name, info) in enumerate(dn.convs()):
            head = info["out0"] < 0
            got = [rgb] if head else _layer_outputs(dn, ci, info)
            for g, (ref, S) in zip(got, _layer_ref(sdh, dw, name, info, dn, layers, x0)):
                ref = ref if head else np.clip(ref, -HALF_MAX, HALF_MAX)
                ulp32 = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                ulp16 = 0.0 if head else np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
                err = np.abs(g.astype(np.float64) - ref)
                assert np.all(err <= 4e-6 * S + 4 * ulp32 + ulp16), (name, float(err.max()))
                over = np.maximum(err - 4 * ulp32 - ulp16, 0.0)
                worst[name] = max(worst.get(name, 0.0), float(np.max(over / np.maximum(S, 1e-30))))
        d_frame.free()
        d_rgb.free()
    finally:
        dn.destroy()
    with capsys.disabled():
        print(f"\n{w}x{h} half per-layer worst (|err| - 4 ulp32 - 1 ulp16) / S:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
        print("overall worst ratio: %.3e (bound 4e-6)" % max(worst.values()))


def test_half_stores_saturate_instead_of_overflowing(pt, lab, gpu, sd):
    """A Cornell frame whose emitter radiance is scaled until the pre-processed colour (radiance / 0.00316 on albedo 0) exceeds
    65504: the stored copy holds exactly 65504 there and the output is finite everywhere."""
    w, h = 100, 75
    frame = cornell(pt, w, h).copy()
    frame[..., 0:3] *= np.float32(1000.0)
    pre = R.preprocess(frame)
    over = pre[..., 0:3] > HALF_MAX
    assert over.any() and np.isfinite(pre).all()
    dn = lab.Denoiser(w, h, sd, precision="half")
    try:
        after = lab.denoise_frame(frame, None, denoiser=dn)
        x0 = dn.activation(0)
        acts = [dn.activation(i) for i in range(len(dn.layers()))]
    finally:
        dn.destroy()
    assert np.all(x0[..., 0:3][over] == np.float32(HALF_MAX))
    want = np.clip(pre, -HALF_MAX, HALF_MAX).astype(np.float16).astype(np.float32)
    assert np.array_equal(bits(x0[..., :14]), bits(want)) and not x0[..., 14:].any()
    assert all(np.isfinite(a).all() and np.abs(a).max() <= HALF_MAX for a in acts)
    assert np.isfinite(after).all() and after[..., 0:3].min() >= 0.0 and after[..., 0:3].max() <= 1.0


def test_half_leaves_frame_channels_3_to_13_as_the_fp32_mode_does(pt, gpu, sd):
    for w, h in ((100, 75), (512, 512)):
        frame = cornell(pt, w, h)
        a32 = pt.denoise_frame(frame, sd)
        a16 = pt.denoise_frame(frame, sd, precision="half")
        assert np.array_equal(bits(a16[..., 3:14]), bits(a32[..., 3:14]))
        assert np.array_equal(bits(a16[..., 3:9]), bits(frame[..., 3:9]))
        assert not np.array_equal(bits(a16[..., 0:3]), bits(a32[..., 0:3]))  # the half mode did run


def _frames(pt, w, h, n):
    base = [pt.render_frame(w, h, spp)[0] for spp in (2, 4)]
    out = np.empty((n, h, w, 14), dtype=np.float32)
    for f in range(n):
        out[f] = base[f % 2]
        out[f, ..., 0:3] *= np.float32(1.0 + 0.05 * f)
    out[1, ..., 9:14] *= np.float32(8.0)  # its maxima differ from its neighbours'
    return out


def test_half_batches_equal_single_enqueues_and_runs_are_deterministic(pt, gpu, sd):
    """enqueue_frames in half mode = the loop of single half enqueues, bit for bit: n = 5 with max_frames 2 and 8 (groups of
    2 + 2 + 1, and one group), gapped strides, odd size 101 x 75, in place and out of place; two runs give the same bits."""
    w, h, n = 101, 75, 5
    px = w * h
    fs, rs = px * 14 + 37, px * 3 + 11
    frames = _frames(pt, w, h, n)
    single = pt.Denoiser(w, h, sd, precision="half")
    try:
        want = np.stack([pt.denoise_frame(frames[f], None, denoiser=single) for f in range(n)])
        want_rgb = np.stack([pt.denoise_frame(frames[f], None, out_of_place=True, denoiser=single)[1] for f in range(n)])
        again = pt.denoise_frame(frames[3], None, denoiser=single)
    finally:
        single.destroy()
    assert np.array_equal(bits(again), bits(want[3]))
    assert np.array_equal(bits(want[..., 0:3]), bits(want_rgb))
    sentinel = np.float32(-1234.5)
    host = np.full(n * fs, sentinel, dtype=np.float32)
    for f in range(n):
        host[f * fs:f * fs + px * 14] = frames[f].ravel()
    for max_frames in (2, 8):
        dn = pt.Denoiser(w, h, sd, max_frames=max_frames, precision="half")
        d = pt.DeviceBuffer(host.nbytes).upload(host)
        d_rgb = pt.DeviceBuffer(n * rs * 4).upload(np.full(n * rs, sentinel, dtype=np.float32))
        try:
            assert dn.precision == "half" and dn.max_frames == max_frames
            dn.denoise_frames(d.ptr, n, frame_stride_floats=fs, d_rgb=d_rgb.ptr, rgb_stride_floats=rs)
            got_rgb = d_rgb.download(np.float32, (n * rs,))
            assert np.array_equal(bits(d.download(np.float32, (n * fs,))), bits(host))  # out of place: frames untouched
            dn.denoise_frames(d.ptr, n, frame_stride_floats=fs)
            got = d.download(np.float32, (n * fs,))
        finally:
            d.free()
            d_rgb.free()
            dn.destroy()
        for f in range(n):
            assert np.array_equal(bits(got[f * fs:f * fs + px * 14]), bits(want[f].ravel())), (max_frames, f)
            assert np.all(got[f * fs + px * 14:(f + 1) * fs] == sentinel)
            assert np.array_equal(bits(got_rgb[f * rs:f * rs + px * 3]), bits(want_rgb[f].ravel())), (max_frames, f)
            assert np.all(got_rgb[f * rs + px * 3:(f + 1) * rs] == sentinel)


def test_half_activation_buffers_are_half_the_bytes(lab, gpu, sd):
    """From the layer table: every activation buffer of a half denoiser is half the bytes of its fp32 twin, 256-byte aligned;
    the split-K partials stay fp32."""
    mem = {}
    for precision in ("float32", "half"):
        dn = lab.Denoiser(512, 512, sd, max_frames=2, precision=precision)
        try:
            mem[precision] = dn.memory()
            shapes = dn.layers()
        finally:
            dn.destroy()
    assert mem["float32"]["element"] == 4 and mem["half"]["element"] == 2
    for (name, off, nbytes), (hname, hoff, hbytes), (_, shape) in zip(mem["float32"]["layers"], mem["half"]["layers"], shapes):
        assert name == hname and nbytes == 4 * int(np.prod(shape)) and 2 * hbytes == nbytes, name
        assert off % 256 == 0 and hoff % 256 == 0
    assert mem["half"]["workspace"] * 2 <= mem["float32"]["workspace"] + 256 * len(shapes)
    assert mem["half"]["weights"] < 0.51 * mem["float32"]["weights"]
    print("\nworkspace bytes (512x512, max_frames 2):", {k: {q: v[q] for q in ("workspace", "partials", "weights")} for k, v in mem.items()})


def test_cli_half_precision_agrees_with_float_within_the_bound(pt, gpu, dw, sd, tmp_path):
    """pathtrace --size 64 -s 4 -d --denoise-weights W --denoise-precision half saves an EXR whose colour differs from the
    float run's and agrees with the float64 network within the end-to-end bound; channels 3-13 are the float run's."""
    wpath = str(tmp_path / "w.ptdn")
    dw.export(sd, wpath)
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    out = {}
    for prec in ("half", "float"):
        o = str(tmp_path / prec)
        run = subprocess.run([exe, "--size", "64", "-s", "4", "-d", "--denoise-weights", wpath, "--denoise-precision", prec, "-o", o,
                              "--nobitmap"], capture_output=True, text=True, timeout=180)
        assert run.returncode == 0, run.stderr
        assert "Denoise completed in" in run.stdout
        out[prec] = _read_exr(o + ".exr", 64, 64)
    assert np.array_equal(bits(out["half"][..., 3:14]), bits(out["float"][..., 3:14]))
    assert not np.array_equal(bits(out["half"][..., 0:3]), bits(out["float"][..., 0:3]))
    frame = cornell(pt, 64, 64)
    ref, model = HM.denoise(frame, sd, None), HM.denoise(frame, sd, "fp16")
    m_max, m_rms = HM.errors(model, ref)
    e_max, e_rms = HM.errors(out["half"][..., 0:3], ref)
    f_max, _ = HM.errors(out["float"][..., 0:3], ref)
    assert f_max <= 1e-4  # the CLI's float run is the fp32 mode on this frame
    assert e_rms <= 2 * m_rms + 1e-5 and e_max <= 3 * m_max + 1e-4, (e_max, e_rms, m_max, m_rms)
