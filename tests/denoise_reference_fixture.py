"""Reader of tests/golden/ref_denoise_*.npz: what the reference's own denoiser code (denoise_cnn/model.py, train.py:test,
load_data.py:get_score) computed on synthetic inputs, recorded by oracle/ref_denoise/record.py.  The files hold data only; the
tests that read them (tests/test_denoiser_reference_host.py, tests/test_denoiser_reference_gpu.py) need neither the reference
nor the recipe's output directory.  Also the one bound both tests share."""
import glob
import hashlib
import os

import numpy as np

from conftest import GOLDEN

PREFIX = "ref_denoise_"
SEED = 3
SIZES = [(1, 1), (7, 5), (19, 13), (37, 29), (64, 48)]  # width x height
PER_MODULE = [(1, 1), (7, 5), (19, 13)]
E2E_BOUND = 1e-4  # tests/test_denoiser_gpu.py: test_end_to_end_against_float64
E32_FACTOR, ULPS = 8.0, 4.0


def tag(w, h):
    return f"{w}x{h}"


def join(flat):
    """{key: array} of the files' entries with the cut arrays ("key#shape", "key#0", "key#1", ...) put together."""
    out = {}
    for key in flat:
        if "#" not in key:
            out[key] = flat[key]
        elif key.endswith("#shape"):
            base = key[:-len("#shape")]
            n = sum(1 for k in flat if k.startswith(base + "#")) - 1
            out[base] = np.concatenate([flat[f"{base}#{i}"] for i in range(n)]).reshape(tuple(flat[key]))
    return out


def load_dir(path):
    flat = {}
    files = sorted(glob.glob(os.path.join(path, PREFIX + "*.npz")))
    for name in files:
        with np.load(name) as z:
            for key in z.files:
                assert key not in flat, key
                flat[key] = z[key]
    return join(flat), files


_cache = {}


def load():
    """The committed recording: {key: array}, read once and left unchanged."""
    if "data" not in _cache:
        data, files = load_dir(GOLDEN)
        assert files, "tests/golden/ref_denoise_*.npz are missing"
        for a in data.values():
            a.setflags(write=False)
        _cache["data"] = data
    return _cache["data"]


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def pre_installed(data, s):
    """The tensor train.py:test() left in place under the installed torch: stored as its distance in float32 steps (at most 2)
    from the 0.2/0.3 recording."""
    base = data[f"{s}/pre_v02"].view(np.int32).astype(np.int64)
    return (base + data[f"{s}/pre_installed_delta"]).astype(np.int32).view(np.float32)


def e32(data, s):
    """{tensor name: max |the reference's float32 run - its float64 run|} for size s."""
    return dict(zip((str(n) for n in data[f"{s}/e32_names"]), (float(v) for v in data[f"{s}/e32_values"])))


def tensors(data, s, run):
    """{module name: recorded tensor [C][h][w]} of one run of size s ("aligned" or "installed")."""
    p = f"{s}/{run}/"
    return {k[len(p):]: v for k, v in data.items() if k.startswith(p)}


_weights = {}


def state_dict(pt_or_module=None):
    """random_state_dict(seed=3), regenerated (101 MB: never stored) once per process."""
    if "sd" not in _weights:
        if pt_or_module is None:
            from cuda_pathtrace_amd import denoise_weights as pt_or_module
        _weights["sd"] = pt_or_module.random_state_dict(seed=SEED)
    return _weights["sd"]


def ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref)).astype(np.float32)).astype(np.float64)


def gpu_bound(ref, e32_of_tensor):
    """The GPU tests' per-tensor bound, elementwise: 8 e32[tensor] + 4 ulp32(ref).  e32 is the reference's own float32 error
    against its float64 run; the factor covers another summation order, split K and the folded batch norm."""
    return E32_FACTOR * e32_of_tensor + ULPS * ulp32(ref)


def hip_view(t):
    """{module name: tensor} (recorded, or tapped from the restatement) -> {name of the GPU's activation buffer: the tensor it
    must hold}: the two outputs of conv1+res_conv are the batch-normed branches, conv2's is the block's output, lat6 and every
    back* hold the ReLU of their convolution, rep_k the upsample + lateral sum, "final" the clamped rgb.  The name of the
    recorded tensor whose e32 applies comes with it."""
    out = {}
    for b in range(1, 7):
        out[f"block{b}.t1"] = (t[f"block{b}.bn1"], f"block{b}.bn1")
        out[f"block{b}.res"] = (t[f"block{b}.res_bn"], f"block{b}.res_bn")
        out[f"block{b}.out"] = (t[f"block{b}"], f"block{b}")
    out["lat6"] = (np.maximum(t["lat_6"], 0), "lat_6")
    for k in range(5, -1, -1):
        out[f"back{k + 1}{k}"] = (np.maximum(t[f"backwards_{k + 1}{k}"], 0), f"backwards_{k + 1}{k}")
        out[f"rep{k}"] = (t[f"upsample_add_{k}"], f"upsample_add_{k}")
    out["final"] = (t["final"], "final")
    return out
