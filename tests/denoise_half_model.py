"""The rounding model of the denoiser's half-precision mode, written from DENOISER.md ("Half precision: where the mode
rounds"), not from the kernels: the float64 restatement (tests/denoise_restatement.py) with a rounding to the storage format
at exactly the points where the mode stores a value --

  * the convolution weights (once; bias and batch-norm parameters stay as they are),
  * the stored copy of the pre-processed frame (the network's input, its albedo channels included),
  * every stored activation: each block's `res_bn` and `bn1` outputs and its sum, `lat_6`, each `backwards` output, each
    upsample + lateral sum,

fp16 stores saturating at +-65504 -- and everything between two stores (convolution sums, bias, ReLU, batch norm, residual
add, bilinear upsample, the head's albedo multiply and clamp) in float64.  The head's output is not rounded (it is written as
float32).  Test infrastructure: the yardstick of the half mode's accuracy bound (tests/test_denoiser_half_*.py)."""
import numpy as np
import torch
import torch.nn.functional as F

import denoise_restatement as R

HALF_MAX = 65504.0
FORMATS = {"fp16": torch.float16, "bf16": torch.bfloat16}


def rounder(fmt):
    """float64 tensor -> the same values rounded (to nearest even, through float32 as the epilogues compute) to `fmt`:
    "fp16" (saturating at +-65504), "bf16", or None (no rounding: the float64 restatement itself)."""
    if fmt is None:
        return lambda t: t
    dt = FORMATS[fmt]

    def q(t):
        if dt == torch.float16:
            t = t.clamp(-HALF_MAX, HALF_MAX)
        return t.to(torch.float32).to(dt).to(torch.float64)

    return q


def forward(x, sd, fmt="fp16"):
    """The network on the pre-processed NCHW float64 input x with the mode's roundings; returns the [0, 1] rgb."""
    q = rounder(fmt)

    def conv(t, name, stride, pad):
        w = torch.as_tensor(np.asarray(sd[name + ".weight"])).double()
        b = torch.as_tensor(np.asarray(sd[name + ".bias"])).double()
        return F.conv2d(t, q(w), b, stride=stride, padding=pad)

    x = q(x)
    raw = [x]
    for b in range(1, 7):
        p = f"block{b}."
        r = q(R.bn(F.relu(conv(raw[-1], p + "res_conv", 2, 1)), sd, p + "res_bn"))
        y = q(R.bn(F.relu(conv(raw[-1], p + "conv1", 2, 1)), sd, p + "bn1"))
        y = R.bn(F.relu(conv(y, p + "conv2", 1, 1)), sd, p + "bn2")
        raw.append(q(y + r))
    rep = q(F.relu(conv(raw[6], "lat_6", 1, 0)))
    for k in range(5, -1, -1):
        rep = q(F.relu(conv(rep, f"backwards_{k + 1}{k}", 2, 1)))
        rep = q(R.upsample(rep, raw[k].shape[2:]) + F.relu(conv(raw[k], f"lat_{k}", 1, 0)))
    out = conv(rep, "rgb_conv", 1, 1)
    return torch.clamp(out * (R.KEPS + x[:, 6:9]), 0, 1)


def denoise(frame, sd, fmt="fp16"):
    """The whole step on a host [H][W][14] frame: rgb [H][W][3] as float64 numpy (fmt=None: tests/denoise_restatement)."""
    f = R.preprocess(frame)
    with torch.no_grad():
        out = forward(R.to_nchw(f, torch.float64), sd, fmt)
    return out[0].permute(1, 2, 0).numpy()


def errors(a, ref):
    """(max abs, rms) of a - ref."""
    e = np.asarray(a, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.abs(e).max()), float(np.sqrt(np.mean(e * e)))


def limits(model, ref):
    """(max abs, rms) a GPU result may differ from the float64 `ref` by, from the model's own error Em = model - ref:
    max |E| <= 3 max |Em| + 1e-4 and rms(E) <= 2 rms(Em) + 1e-5.  Kernel and model are two draws of the same rounding process
    (fp32 instead of float64 sums flip individual fp16 roundings); a bf16-sized error (3 x and more in rms) fails."""
    m_max, m_rms = errors(model, ref)
    return 3 * m_max + 1e-4, 2 * m_rms + 1e-5
