"""Weights of the reference's denoising network (DenoiseCNN, denoise_cnn/model.py) in the library's PTDN file format.

The reference ships no trained weights: users bring a state_dict trained with its train.py, keyed by its parameter names
(block1.res_conv.weight, block1.res_bn.running_var, ..., lat_0.bias, backwards_10.weight, rgb_conv.weight).  export() writes
such a state_dict as a PTDN file (layout: include/ptcore.h, "denoiser"); the library's loader checks every key and shape.
numpy only: torch tensors are accepted (anything with .detach().cpu().numpy() or np.asarray), torch is not needed.
"""
import struct

import numpy as np

MAGIC = b"PTDN"
VERSION = 1
BN_EPS = 1e-5
CHANNELS = (14, 32, 64, 128, 256, 512, 1024)  # C_0 (the pre-processed frame) .. C_6


def expected_shapes():
    """name -> shape of every tensor the network needs, in the order export() writes them."""
    out = {}
    for b in range(1, 7):
        cin, cout = CHANNELS[b - 1], CHANNELS[b]
        for conv, ci in (("res_conv", cin), ("conv1", cin), ("conv2", cout)):
            out[f"block{b}.{conv}.weight"] = (cout, ci, 3, 3)
            out[f"block{b}.{conv}.bias"] = (cout,)
        for bn in ("res_bn", "bn1", "bn2"):
            for p in ("weight", "bias", "running_mean", "running_var"):
                out[f"block{b}.{bn}.{p}"] = (cout,)
    for k in range(6, -1, -1):
        out[f"lat_{k}.weight"] = (32, CHANNELS[k], 1, 1)
        out[f"lat_{k}.bias"] = (32,)
        if k < 6:
            out[f"backwards_{k + 1}{k}.weight"] = (32, 32, 3, 3)
            out[f"backwards_{k + 1}{k}.bias"] = (32,)
    out["rgb_conv.weight"] = (3, 32, 3, 3)
    out["rgb_conv.bias"] = (3,)
    return out


def _array(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype="<f4")


def to_bytes(state_dict):
    """The PTDN image of a reference-keyed state_dict (num_batches_tracked entries are dropped).  Keys and shapes are written
    as given: the library's loader, not this function, decides whether they are complete and right."""
    items = [(k, _array(v)) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")]
    parts = [MAGIC, struct.pack("<II", VERSION, len(items))]
    for name, a in items:
        nb = name.encode("utf-8")
        parts.append(struct.pack("<I", len(nb)) + nb + struct.pack("<I", a.ndim) + struct.pack(f"<{a.ndim}I", *a.shape))
        parts.append(a.tobytes())
    return b"".join(parts)


def export(state_dict, path):
    """Write a reference-keyed state_dict as a PTDN file."""
    with open(path, "wb") as f:
        f.write(to_bytes(state_dict))


def from_bytes(blob):
    """Parse a PTDN image back into {name: float32 array} (no completeness check: see the library's pt_denoiser_weights_check)."""
    blob = bytes(blob)
    if blob[:4] != MAGIC:
        raise ValueError("not a PTDN file")
    version, n = struct.unpack_from("<II", blob, 4)
    if version != VERSION:
        raise ValueError(f"PTDN version {version}")
    off, out = 12, {}
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", blob, off)
        name = blob[off + 4:off + 4 + ln].decode("utf-8")
        off += 4 + ln
        (nd,) = struct.unpack_from("<I", blob, off)
        shape = struct.unpack_from(f"<{nd}I", blob, off + 4)
        off += 4 + 4 * nd
        cnt = int(np.prod(shape)) if nd else 1
        out[name] = np.frombuffer(blob, dtype="<f4", count=cnt, offset=off).reshape(shape).copy()
        off += 4 * cnt
    if off != len(blob):
        raise ValueError("trailing bytes")
    return out


def random_state_dict(seed=0, rgb_scale=0.003, integer=False):
    """Test weights for every tensor of expected_shapes().

    Default: He-scaled normal conv weights (std sqrt(2 / fan_in)), small biases, and batch-norm statistics that are NOT the
    identity -- running mean near 0, running var, gamma and beta near 1 but never equal to it -- so that the folded BN epilogue
    is exercised.  rgb_scale scales the rgb_conv head so that a useful share of the outputs lands inside the clamp to [0, 1].
    integer=True: small ASYMMETRIC integer conv weights (-3..3, skewed) and integer biases, for exact-arithmetic tests of the
    GEMM lane maps (every partial sum of integer activations is then exact in float32)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in expected_shapes().items():
        if name.endswith(".running_mean"):
            a = rng.normal(0.0, 0.1, shape)
        elif name.endswith(".running_var"):
            a = rng.uniform(0.6, 1.4, shape)
        elif name.endswith("_bn.weight") or ".bn1.weight" in name or ".bn2.weight" in name:
            a = rng.uniform(0.8, 1.2, shape)
        elif name.endswith("_bn.bias") or ".bn1.bias" in name or ".bn2.bias" in name:
            a = 1.0 + rng.normal(0.0, 0.1, shape)
        elif name.endswith(".weight"):
            if integer:
                a = rng.choice(np.array([-3, -2, -1, 0, 1, 1, 2, 3, 3]), size=shape)
            else:
                fan_in = int(np.prod(shape[1:]))
                a = rng.normal(0.0, np.sqrt(2.0 / fan_in), shape)
                if name.startswith("rgb_conv"):
                    a = a * rgb_scale
        else:  # conv bias
            a = rng.integers(-4, 5, shape) if integer else rng.normal(0.0, 0.02, shape)
        out[name] = np.asarray(a, dtype=np.float32)
    return out


def fold_bn(sd, bn):
    """The folded affine y = x * scale + shift the library applies for batch-norm `bn` (eval mode, eps 1e-5), computed in
    float64 and rounded once: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    g = sd[bn + ".weight"].astype(np.float64)
    b = sd[bn + ".bias"].astype(np.float64)
    m = sd[bn + ".running_mean"].astype(np.float64)
    v = sd[bn + ".running_var"].astype(np.float64)
    s = g / np.sqrt(v + BN_EPS)
    return s.astype(np.float32), (b - m * s).astype(np.float32)
