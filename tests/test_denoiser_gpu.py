"""The denoising network on the GPU (pt_denoiser_*, csrc/pt_denoise.hip) against a float64 torch CPU restatement written
from the specification (tests/denoise_restatement.py): exact pre-processing, exact MFMA lane maps on integer data, a sound
per-layer rounding bound, end-to-end error, odd shapes, the in-place / out-of-place modes, determinism and the CLI's -d."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import denoise_restatement as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXR_SOURCE = [8, 7, 6, 12, 2, 1, 0, 10, 9, 13, 5, 4, 3, 11]  # host/ExrWriter.h: frame channel of each EXR channel


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


@pytest.fixture(scope="module")
def sd(dw):
    return dw.random_state_dict(seed=1)


_frames = {}


def cornell(pt, w, h, spp=4):
    if (w, h, spp) not in _frames:
        _frames[(w, h, spp)] = pt.render_frame(w, h, spp)[0]
    return _frames[(w, h, spp)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_preprocess_is_exact(pt, lab, gpu, sd):
    """Channels 9-13 of the in-place frame and the colour / albedo division the network reads equal numpy float32 bit for
    bit (divisor of 9-13 formed in double, torch 0.2/0.3); channels 3-8 are untouched."""
    for w, h in ((100, 75), (512, 512)):
        frame = cornell(pt, w, h)
        ref = R.preprocess(frame)
        dn = lab.Denoiser(w, h, sd)
        try:
            after = lab.denoise_frame(frame, None, denoiser=dn)
            x0 = dn.activation(0)
        finally:
            dn.destroy()
        assert np.array_equal(bits(after[..., 9:14]), bits(ref[..., 9:14]))
        assert np.array_equal(bits(after[..., 3:9]), bits(frame[..., 3:9]))
        assert np.array_equal(bits(x0[..., :14]), bits(ref)) and not x0[..., 14:].any()


def test_preprocess_finds_maxima_in_every_trip_of_the_reduction(pt, gpu, sd):
    """520 x 516 (256 workgroups of pre_max_kernel, five trips each), the maxima of channels 9-13 planted where the scene never
    puts them (tests/stage_sum_cases.py): the start of the second trip, the last pixel, the end of the first trip, pixel 0, the
    third trip.  Channels 9-13 of the in-place frame have the restatement's bits."""
    import stage_sum_cases as sc

    frame = sc.patches_planted()[0]
    with np.errstate(all="ignore"):
        ref = R.preprocess(frame)
    after = pt.denoise_frame(frame, sd)
    for c in range(9, 14):
        assert ref[..., c].max() == np.float32(sc.PLANTED_VALUES[c]) / np.float32(0.00316 + sc.PLANTED_VALUES[c])
        bad = np.argwhere(bits(after[..., c]) != bits(ref[..., c]))
        assert len(bad) == 0, f"channel {c} (maximum at pixel {sc.PLANTED[c]}): {len(bad)} differ, first (y, x) = {bad[0].tolist()}"
    assert np.array_equal(bits(after[..., 3:9]), bits(frame[..., 3:9]))


def _conv_ref64(x, w, stride, ks):
    """float64 conv of NHWC x with torch weight w (no bias): NHWC result."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(2, 0, 1).unsqueeze(0)
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64))
    y = F.conv2d(xt, wt, stride=stride, padding=ks // 2)
    return y[0].permute(1, 2, 0).numpy()


def _pad_input_weight(w, cin_stored):
    if w.shape[1] == cin_stored:
        return w
    out = np.zeros((w.shape[0], cin_stored) + w.shape[2:], dtype=w.dtype)
    out[:, :w.shape[1]] = w
    return out


def _torch_names(name):
    """torch conv name(s) and BN name(s) behind a library convolution."""
    if name.endswith("conv1+res_conv"):
        b = name.split(".")[0]
        return [(b + ".conv1", b + ".bn1"), (b + ".res_conv", b + ".res_bn")]
    if name.endswith(".conv2"):
        b = name.split(".")[0]
        return [(b + ".conv2", b + ".bn2")]
    return [(name, None)]


def _layer_outputs(dn, ci, info):
    outs = [info["out0"]] + ([info["out1"]] if info["out1"] >= 0 else [])
    return [dn.activation(o) for o in outs]


def test_mfma_lane_maps_are_exact_on_integer_data(pt, lab, gpu, dw):
    """One layer of each kind and every tile shape, on small-integer activations and ASYMMETRIC integer weights (every sum
    exact in fp32): the layer output equals the float64 restatement bit for bit, whatever the summation order.  A transposed
    or mis-tapped fragment, a wrong C/D row map or a lost split-K slice fails outright."""
    sdi = dw.random_state_dict(seed=5, integer=True)
    rs = np.random.default_rng(9)
    picks = {256: ["block1.conv1+res_conv", "block1.conv2", "block2.conv1+res_conv", "lat_6", "block6.conv1+res_conv",
                   "block6.conv2", "backwards_10", "backwards_65"],
             1024: ["block3.conv1+res_conv", "block1.conv2"]}
    seen_tiles, seen_split = set(), False
    for size, names in picks.items():
        dn = lab.Denoiser(size, size, sdi)
        try:
            layers = dn.layers()
            convs = {n: (i, inf) for i, (n, inf) in enumerate(dn.convs())}
            for name in names:
                ci, info = convs[name]
                shape = layers[info["in"]][1]
                x = rs.choice(np.array([-2, -1, 0, 1, 1, 2], dtype=np.float32), size=shape)
                dn.set_activation(info["in"], x)
                res = None
                if info["res"] >= 0:
                    res = rs.integers(-3, 4, size=layers[info["res"]][1]).astype(np.float32)
                    dn.set_activation(info["res"], res)
                dn.run_conv(ci)
                got = _layer_outputs(dn, ci, info)
                for k, (tname, bn) in enumerate(_torch_names(name)):
                    wgt = _pad_input_weight(sdi[tname + ".weight"], shape[2])
                    acc = _conv_ref64(x, wgt, info["stride"], info["ks"])
                    v = np.maximum(acc + sdi[tname + ".bias"].astype(np.float64), 0.0)
                    if bn:
                        s, t = dw.fold_bn(sdi, bn)
                        v = v * s.astype(np.float64) + t.astype(np.float64)  # exact in float64 here: one rounding = the fma
                    ref = v.astype(np.float32)
                    if res is not None:
                        ref = ref + res
                    g = got[k]
                    assert g.shape == ref.shape, name
                    bad = np.argwhere(bits(g) != bits(ref))
                    assert len(bad) == 0, f"{name}: {len(bad)} differ, first {bad[:3].tolist()} {g[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
                seen_tiles.add((info["bm"], info["bn"]))
                seen_split |= info["splits"] > 1
        finally:
            dn.destroy()
    assert seen_tiles == {(256, 32), (128, 64), (128, 128), (128, 32), (64, 64)} and seen_split, seen_tiles


def _layer_ref(sd, dw, name, info, dn, layers, frame_in):
    """float64 output(s) of one convolution from the HIP input(s) of that layer, and the scale S of the bound."""
    x = dn.activation(info["in"]).astype(np.float64)
    outs = []
    for tname, bn in _torch_names(name):
        wgt = _pad_input_weight(sd[tname + ".weight"], x.shape[2]).astype(np.float64)
        b = sd[tname + ".bias"].astype(np.float64)
        acc = _conv_ref64(x, wgt, info["stride"], info["ks"]) + b
        S = _conv_ref64(np.abs(x), np.abs(wgt), info["stride"], info["ks"]) + np.abs(b)
        if info["epi"] == 0:
            v = np.maximum(acc, 0.0)
            if bn:
                g, be = sd[bn + ".weight"].astype(np.float64), sd[bn + ".bias"].astype(np.float64)
                m, var = sd[bn + ".running_mean"].astype(np.float64), sd[bn + ".running_var"].astype(np.float64)
                sc = g / np.sqrt(var + 1e-5)
                v = (v - m) / np.sqrt(var + 1e-5) * g + be
                S = S * np.abs(sc)
            if info["res"] >= 0:
                r = dn.activation(info["res"]).astype(np.float64)
                v, S = v + r, S + np.abs(r)
        elif info["epi"] == 1:
            up = torch.from_numpy(dn.activation(info["up"]).astype(np.float64)).permute(2, 0, 1).unsqueeze(0)
            u = R.upsample(up, x.shape[:2])[0].permute(1, 2, 0).numpy()
            ua = R.upsample(up.abs(), x.shape[:2])[0].permute(1, 2, 0).numpy()
            v, S = u + np.maximum(acc, 0.0), S + ua
        else:
            alb = R.KEPS + frame_in[..., 6:9].astype(np.float64)
            v, S = np.clip(acc * alb, 0.0, 1.0), S * alb
        outs.append((v, S))
    return outs


def test_per_layer_rounding_within_the_bound(pt, lab, gpu, dw, sd, capsys):
    """Every layer, from the HIP input of that layer: |hip - ref| <= 4e-6 S + 4 ulp(ref), S = conv(|x|, |W|) + |bias| scaled
    by |BN scale| (+ |residual| / the upsampled |coarse map| where the epilogue adds one).  Reports the worst ratio.  At
    256 x 256 and at 37 x 29 (every M ragged, maps down to 1 x 1), the same bound."""
    for w, h in ((256, 256), (37, 29)):
        _per_layer_rounding(pt, lab, dw, sd, capsys, w, h)


def _per_layer_rounding(pt, lab, dw, sd, capsys, w, h):
    frame = cornell(pt, w, h)
    dn = lab.Denoiser(w, h, sd)
    worst = {}
    try:
        d_frame = lab.DeviceBuffer(frame.nbytes).upload(frame)
        d_rgb = lab.DeviceBuffer(w * h * 12)
        dn.denoise(d_frame.ptr, d_rgb.ptr)
        rgb = d_rgb.download(np.float32, (h, w, 3))
        layers = dn.layers()
        for ci, (name, info) in enumerate(dn.convs()):
            got = [rgb] if info["out0"] < 0 else _layer_outputs(dn, ci, info)
            for g, (ref, S) in zip(got, _layer_ref(sd, dw, name, info, dn, layers, frame)):
                ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                err = np.abs(g.astype(np.float64) - ref)
                assert np.all(err <= 4e-6 * S + 4 * ulp), (name, float(err.max()))
                over = np.maximum(err - 4 * ulp, 0.0)
                worst[name] = max(worst.get(name, 0.0), float(np.max(over / np.maximum(S, 1e-30))))
        d_frame.free()
        d_rgb.free()
    finally:
        dn.destroy()
    with capsys.disabled():
        print(f"\n{w}x{h} per-layer worst (|err| - 4 ulp) / S:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
        print("overall worst ratio: %.3e (bound 4e-6)" % max(worst.values()))


@pytest.mark.parametrize("w,h", [(512, 512), (1, 1), (7, 5), (100, 75), (1024, 1024)])
def test_end_to_end_against_float64(pt, gpu, sd, w, h, capsys):
    """Rendered Cornell frame, random weights: max |hip - float64| <= 1e-4 on the [0, 1] output; at the full sizes at least
    30 % of the outputs are unclamped (the generator scales rgb_conv so that this holds)."""
    frame = cornell(pt, w, h)
    after = pt.denoise_frame(frame, sd)
    pre, ref = R.denoise(frame, sd)
    err = float(np.abs(after[..., 0:3].astype(np.float64) - ref).max())
    unclamped = float(((ref > 0) & (ref < 1)).mean())
    with capsys.disabled():
        print(f"\n{w}x{h}: max |err| {err:.3e}, unclamped {unclamped:.3f}")
    assert err <= 1e-4
    if w * h >= 100 * 75:
        assert unclamped >= 0.30
    assert np.array_equal(bits(after[..., 3:14]), bits(pre[..., 3:14]))


def test_modes_determinism_and_side_by_side_denoisers(pt, gpu, sd):
    frame = cornell(pt, 100, 75)
    dn = pt.Denoiser(100, 75, sd)
    small = pt.Denoiser(64, 48, sd)
    try:
        untouched, rgb = pt.denoise_frame(frame, None, out_of_place=True, denoiser=dn)
        assert np.array_equal(bits(untouched), bits(frame))
        f_small = cornell(pt, 64, 48)
        a_small = pt.denoise_frame(f_small, None, denoiser=small)
        a = pt.denoise_frame(frame, None, denoiser=dn)
        b = pt.denoise_frame(frame, None, denoiser=dn)
        b_small = pt.denoise_frame(f_small, None, denoiser=small)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a_small), bits(b_small))
        assert np.array_equal(bits(a[..., 0:3]), bits(rgb))
        alone = pt.denoise_frame(f_small, sd)
        assert np.array_equal(bits(alone), bits(a_small))
    finally:
        dn.destroy()
        small.destroy()
    # the split-K layers are deterministic at the size where they matter most
    big = cornell(pt, 512, 512)
    dn = pt.Denoiser(512, 512, sd)
    try:
        r1 = pt.denoise_frame(big, None, denoiser=dn)
        r2 = pt.denoise_frame(big, None, denoiser=dn)
    finally:
        dn.destroy()
    assert np.array_equal(bits(r1), bits(r2))


def _read_exr(path, w, h):
    raw = open(path, "rb").read()
    block = 8 + w * 14 * 4
    data = raw[len(raw) - h * block:]
    out = np.empty((h, w, 14), np.float32)
    for y in range(h):
        row = np.frombuffer(data, dtype="<f4", count=w * 14, offset=y * block + 8).reshape(14, w)
        for c in range(14):
            out[y, :, EXR_SOURCE[c]] = row[c]
    return out


def test_cli_denoises_the_frame_loop(pt, gpu, dw, sd, tmp_path):
    """pathtrace --size 96 --frames 2 -d --denoise-weights W: the saved EXR is the second frame after the network in place,
    bit for bit what the Python API computes from the same two renders; --preview packs the denoised colour."""
    wpath = str(tmp_path / "w.ptdn")
    dw.export(sd, wpath)
    out, ppm = str(tmp_path / "dn"), str(tmp_path / "dn.ppm")
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    run = subprocess.run([exe, "--size", "96", "--frames", "2", "-d", "--denoise-weights", wpath, "-o", out, "--nobitmap",
                          "--preview", ppm], capture_output=True, text=True, timeout=180)
    assert run.returncode == 0, run.stderr
    assert "Denoise completed in" in run.stdout
    got = _read_exr(out + ".exr", 96, 96)
    r = pt.Renderer(96, 96, 4)
    d_scene, n = pt.upload_scene(pt.scene_cornell())
    d_out = pt.DeviceBuffer(96 * 96 * 56)
    dn = pt.Denoiser(96, 96, sd)
    try:
        basis = pt.camera_basis(width=96, height=96)
        r.render(d_out.ptr, d_scene.ptr, n, basis)
        dn.denoise(d_out.ptr)
        r.render(d_out.ptr, d_scene.ptr, n, basis)
        dn.denoise(d_out.ptr)
        want = d_out.download(np.float32, (96, 96, 14))
    finally:
        dn.destroy()
        r.destroy()
    assert np.array_equal(bits(got), bits(want))
    packed = pt.display_pack(want)
    rgba = packed[..., 2].copy().view(np.uint8).reshape(96, 96, 4)[..., :3]
    body = open(ppm, "rb").read()
    assert body.startswith(b"P6\n96 96\n255\n") and body[len(b"P6\n96 96\n255\n"):] == rgba.tobytes()
