"""A float64 torch (CPU) restatement of the reference's denoising step, written from the specification in DENOISER.md
(pre-processing of train.py:test, DenoiseCNN's eval-mode forward, modify_tensor), not from the reference's code -- and held
to what the reference's code computes, tensor by tensor, by tests/test_denoiser_reference_host.py (recordings of
oracle/ref_denoise/record.py under tests/golden/).
Test infrastructure: tests/test_denoiser_*.py and tools/denoise_time.py (its fp32 comparison point)."""
import numpy as np
import torch
import torch.nn.functional as F

KEPS = 0.00316
BN_EPS = 1e-5


def preprocess(frame):
    """train.py:48-55 on a float32 [H][W][14] frame, in float32 as the reference computes it: colour / (0.00316f + albedo);
    channel k of 9-13 / (float)(0.00316 + (double)max_k) -- torch 0.2/0.3's torch.max(t) returned a Python float."""
    f = np.array(frame, dtype=np.float32, copy=True)
    f[..., 0:3] = f[..., 0:3] / (np.float32(KEPS) + f[..., 6:9])
    for k in range(9, 14):
        f[..., k] = f[..., k] / np.float32(KEPS + float(f[..., k].max()))
    return f


def to_nchw(f, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(f)).to(dtype).permute(2, 0, 1).unsqueeze(0).contiguous()


def _t(sd, name, like):
    v = sd[name]
    t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
    return t.to(dtype=like.dtype, device=like.device)


def conv(x, sd, name, stride, pad):
    return F.conv2d(x, _t(sd, name + ".weight", x), _t(sd, name + ".bias", x), stride=stride, padding=pad)


def bn(x, sd, name):
    """BatchNorm2d in eval mode: (x - running_mean) / sqrt(running_var + eps) * gamma + beta."""
    sh = (1, -1, 1, 1)
    m, v = _t(sd, name + ".running_mean", x).view(sh), _t(sd, name + ".running_var", x).view(sh)
    g, b = _t(sd, name + ".weight", x).view(sh), _t(sd, name + ".bias", x).view(sh)
    return (x - m) / torch.sqrt(v + BN_EPS) * g + b


def _tap(tap, name, t):
    if tap is not None:
        tap(name, t)
    return t


def resblock(x, sd, b, tap=None):
    """ResBlock: r = BN_res(ReLU(conv_s2_res(x))), y = BN2(ReLU(conv_s1(BN1(ReLU(conv_s2(x)))))), out = y + r.  tap(name, tensor)
    sees every module's output under the reference's module name."""
    p = f"block{b}."
    r = _tap(tap, p + "res_conv", conv(x, sd, p + "res_conv", 2, 1))
    r = _tap(tap, p + "res_bn", bn(F.relu(r), sd, p + "res_bn"))
    y = _tap(tap, p + "conv1", conv(x, sd, p + "conv1", 2, 1))
    y = _tap(tap, p + "bn1", bn(F.relu(y), sd, p + "bn1"))
    y = _tap(tap, p + "conv2", conv(y, sd, p + "conv2", 1, 1))
    y = _tap(tap, p + "bn2", bn(F.relu(y), sd, p + "bn2"))
    return _tap(tap, f"block{b}", y + r)


def upsample(x, size, align_corners=True):
    """F.upsample(mode='bilinear') of torch 0.2/0.3: align-corners semantics (align_corners=False: what the same call means
    to a torch of today, tests/test_denoiser_reference_host.py)."""
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=align_corners)


def forward(x, sd, align_corners=True, tap=None):
    """The network on the pre-processed NCHW input x; returns clamp(rgb_conv(rep) * (0.00316 + x[:, 6:9]), 0, 1).
    tap(name, tensor): every module's output (convolutions before their ReLU), each upsample + lateral sum as
    "upsample_add_k", the head times the albedo term as "preclamp" and the result as "final"."""
    raw = [x]
    for b in range(1, 7):
        raw.append(resblock(raw[-1], sd, b, tap))
    rep = F.relu(_tap(tap, "lat_6", conv(raw[6], sd, "lat_6", 1, 0)))
    for k in range(5, -1, -1):
        rep = F.relu(_tap(tap, f"backwards_{k + 1}{k}", conv(rep, sd, f"backwards_{k + 1}{k}", 2, 1)))
        lat = F.relu(_tap(tap, f"lat_{k}", conv(raw[k], sd, f"lat_{k}", 1, 0)))
        rep = _tap(tap, f"upsample_add_{k}", upsample(rep, raw[k].shape[2:], align_corners) + lat)
    out = _tap(tap, "rgb_conv", conv(rep, sd, "rgb_conv", 1, 1))
    pre = _tap(tap, "preclamp", out * (KEPS + x[:, 6:9]))
    return _tap(tap, "final", torch.clamp(pre, 0, 1))


def denoise(frame, sd, dtype=torch.float64):
    """The whole step on a host frame: (pre-processed frame, rgb [H][W][3] as float64 numpy)."""
    f = preprocess(frame)
    with torch.no_grad():
        out = forward(to_nchw(f, dtype), sd)
    return f, out[0].permute(1, 2, 0).double().numpy()
