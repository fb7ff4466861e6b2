"""A float64 torch (CPU) restatement of the reference's denoising step, written from the specification in DENOISER.md
(pre-processing of train.py:test, DenoiseCNN's eval-mode forward, modify_tensor), not from the reference's code.
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


def resblock(x, sd, b):
    """ResBlock: r = BN_res(ReLU(conv_s2_res(x))), y = BN2(ReLU(conv_s1(BN1(ReLU(conv_s2(x)))))), out = y + r."""
    p = f"block{b}."
    r = bn(F.relu(conv(x, sd, p + "res_conv", 2, 1)), sd, p + "res_bn")
    y = bn(F.relu(conv(x, sd, p + "conv1", 2, 1)), sd, p + "bn1")
    y = bn(F.relu(conv(y, sd, p + "conv2", 1, 1)), sd, p + "bn2")
    return y + r


def upsample(x, size):
    """F.upsample(mode='bilinear') of torch 0.2/0.3: align-corners semantics."""
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


def forward(x, sd):
    """The network on the pre-processed NCHW input x; returns clamp(rgb_conv(rep) * (0.00316 + x[:, 6:9]), 0, 1)."""
    raw = [x]
    for b in range(1, 7):
        raw.append(resblock(raw[-1], sd, b))
    rep = F.relu(conv(raw[6], sd, "lat_6", 1, 0))
    for k in range(5, -1, -1):
        rep = F.relu(conv(rep, sd, f"backwards_{k + 1}{k}", 2, 1))
        rep = upsample(rep, raw[k].shape[2:]) + F.relu(conv(raw[k], sd, f"lat_{k}", 1, 0))
    out = conv(rep, sd, "rgb_conv", 1, 1)
    return torch.clamp(out * (KEPS + x[:, 6:9]), 0, 1)


def denoise(frame, sd, dtype=torch.float64):
    """The whole step on a host frame: (pre-processed frame, rgb [H][W][3] as float64 numpy)."""
    f = preprocess(frame)
    with torch.no_grad():
        out = forward(to_nchw(f, dtype), sd)
    return f, out[0].permute(1, 2, 0).double().numpy()
