#!/usr/bin/env python3
"""Records what the reference's own denoiser code computes, for tests/golden/ref_denoise_*.npz.

The reference's denoiser is Python and runs on the CPU.  This recipe executes its program text IN PLACE and copies none of it:
DenoiseCNN is imported from denoise_cnn/model.py; train.py and load_data.py cannot be imported (OpenEXR and Imath are absent,
train.py sets CUDA variables at import), so the single functions `test` and `get_score` are taken out of the parsed files and
compiled alone into a namespace that holds `torch` or `np`.  Nothing is written into the reference tree (no bytecode either);
the output goes to oracle/_ref/denoise/, which stays out of git.  `python tests/golden/make_golden.py ref_denoise` copies it to
tests/golden/.

Every synthetic input (inputs(), below) goes through the network three ways, with random_state_dict(seed=3) loaded, eval():

  aligned    float64, torch.nn.functional.upsample given its torch 0.2/0.3 meaning (align_corners=True) for the run;
  installed  float64, the same call as the installed torch runs it (align_corners=False);
  f32        float32 with aligned upsampling: the precision the reference itself runs at.

Per run: the output of every module (forward hooks), the result of every _upsample_add (the bound method wrapped on the
instance), the argument of the final torch.clamp (the pre-clamp rgb: the recording keeps what the clamp would hide) and the return value.  For
every tensor e32 = max |f32 - aligned|: the reference's own float32 error, the yardstick of the GPU tests.

train.py:test() runs twice on every input in float32: as installed, and with the namespace's torch.max returning a Python
float as torch 0.2/0.3 did (aligned upsampling with it).  load_data.py:get_score runs on patches of the pre-processed frame.
"""
import argparse
import ast
import contextlib
import hashlib
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference/denoise_cnn"
OUT = os.path.join(ROOT, "oracle", "_ref", "denoise")
PREFIX = "ref_denoise_"
LIMIT = 133256  # bytes: no fixture file may be larger than the largest one tests/golden held before these
CHUNK = 120000  # bytes of array data per file (compression only shrinks it; the zip directory adds a little)

SEED = 3
SIZES = ((1, 1), (7, 5), (19, 13), (37, 29), (64, 48))  # width x height
PER_MODULE = ((1, 1), (7, 5), (19, 13))  # sizes whose per-module tensors are kept
SCORE_PATCHES = (8, 16)
KEPS = 0.00316


def tag(w, h):
    return f"{w}x{h}"


def available():
    return os.path.exists(os.path.join(REFERENCE, "model.py"))


def denoise_weights():
    """cuda-pathtrace_amd/denoise_weights.py (numpy only), without loading the native library."""
    name = "_ref_denoise_weights"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "cuda-pathtrace_amd", "denoise_weights.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules[name] = mod
    return sys.modules[name]


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()


# ---- the inputs -----------------------------------------------------------------------------------------------------------

def make_input(w, h):
    """A synthetic float32 [H][W][14] frame: HDR lognormal colour, unit normals, albedo in [0, 1] with exact zeros, channels
    9-13 non-negative with maxima spread over 1e-4 .. 10 (a small maximum is where 0.00316 + max rounds differently in float32
    and in double)."""
    rng = np.random.default_rng(1000 * w + h)
    f = np.empty((h, w, 14), np.float32)
    base = np.exp(rng.normal(-3.2, 1.2, (h, w, 3)))
    f[..., 0:3] = np.minimum(base * np.exp(rng.normal(0.0, 0.5, base.shape)), 100.0)
    n = rng.normal(0.0, 1.0, (h, w, 3))
    f[..., 3:6] = n / np.linalg.norm(n, axis=2, keepdims=True)
    alb = rng.uniform(0.0, 1.0, (h, w, 3))
    alb[rng.random((h, w, 3)) < 0.1] = 0.0
    if w * h >= 35:
        alb[h // 2, w // 2] = 0.0
    f[..., 6:9] = alb
    top = 10.0 ** rng.permutation(np.linspace(-4.0, 1.0, 5))
    f[..., 9:14] = rng.uniform(0.0, 1.0, (h, w, 5)) * top
    return f


def inputs():
    return {(w, h): make_input(w, h) for w, h in SIZES}


def weights():
    """(state_dict of torch float32 tensors, SHA-256 of its PTDN bytes)."""
    dw = denoise_weights()
    sd = dw.random_state_dict(seed=SEED)
    return {k: torch.from_numpy(v) for k, v in sd.items()}, sha256(dw.to_bytes(sd))


# ---- the reference's code, in place ---------------------------------------------------------------------------------------

@contextlib.contextmanager
def _no_bytecode():
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        yield
    finally:
        sys.dont_write_bytecode = old


def reference_model_class():
    with _no_bytecode():
        spec = importlib.util.spec_from_file_location("_ref_denoise_cnn_model", os.path.join(REFERENCE, "model.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod.DenoiseCNN


def reference_function(filename, name, namespace):
    """The one FunctionDef `name` of the reference's `filename`, compiled alone into `namespace`."""
    path = os.path.join(REFERENCE, filename)
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1, (filename, name)
    exec(compile(ast.Module(body=found, type_ignores=[]), path, "exec"), namespace)
    return namespace[name]


def reference_model(sd, dtype):
    model = reference_model_class()()
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    model.eval()
    return model.to(dtype)


def _aligned_upsample(input, size=None, scale_factor=None, mode="nearest", align_corners=None):
    return F.interpolate(input, size=size, scale_factor=scale_factor, mode=mode, align_corners=True)


@contextlib.contextmanager
def upsampling(aligned):
    """torch.nn.functional.upsample with its torch 0.2/0.3 meaning for the duration, or as installed."""
    old = F.upsample
    if aligned:
        F.upsample = _aligned_upsample
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            yield
    finally:
        F.upsample = old


def run_network(model, x, aligned):
    """model(x) with every module's output, every _upsample_add result, the clamp's argument and the result recorded.
    For the duration of the call torch.clamp and torch.nn.functional.upsample are replaced ON THE torch MODULES THEMSELVES
    (the reference looks them up there at call time) and restored in `finally`: nothing else in the process may use torch
    concurrently -- the recipe and the tests that call this are single-threaded."""
    rec, hooks = {}, []

    def keep(name):
        def hook(_mod, _inp, out):
            rec[name] = out.detach().clone()
        return hook

    for name, m in model.named_modules():
        if name and not isinstance(m, torch.nn.ReLU):  # (the one ReLU instance is shared by every call site)
            hooks.append(m.register_forward_hook(keep(name)))
    bound, level = model._upsample_add, [5]

    def upsample_add(a, b):
        out = bound(a, b)
        rec[f"upsample_add_{level[0]}"] = out.detach().clone()
        level[0] -= 1
        return out

    clamp = torch.clamp

    def keep_clamp(t, *args, **kw):
        rec["preclamp"] = t.detach().clone()
        return clamp(t, *args, **kw)

    model._upsample_add = upsample_add
    torch.clamp = keep_clamp
    try:
        with torch.no_grad(), upsampling(aligned):
            rec["final"] = model(x).detach().clone()
    finally:
        torch.clamp = clamp
        del model._upsample_add
        for hk in hooks:
            hk.remove()
    assert level[0] == -1 and "preclamp" in rec
    return rec


class _OldTorch:
    """`torch` as test() sees it under the 0.2/0.3 reading: torch.max(t) returns a Python float."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def max(t):
        return float(torch.max(t))


def run_test(test_fn, model, frame, aligned):
    """train.py:test(model, boost_tensor) on a copy of the [H][W][14] frame: (the in-place pre-processed tensor, rgb)."""
    t = torch.from_numpy(np.array(frame, dtype=np.float32, copy=True))
    with torch.no_grad(), upsampling(aligned):
        out = test_fn(model, t)
    return t.numpy().copy(), out.detach().numpy().copy()


def corners(w, h, p):
    """(x, y) corners of P x P patches: the four extremes (the frame's last row and column among them) and an odd inner one."""
    mx, my = w - p, h - p
    return sorted({(0, 0), (mx, my), (mx, 0), (0, my), (min(3, mx), min(1, my))})


# ---- the recording --------------------------------------------------------------------------------------------------------

def nchw(pre, dtype):
    """[H][W][14] -> (1, 14, H, W) the way test() does it: unsqueeze and permute, the memory stays as it lies."""
    return torch.unsqueeze(torch.from_numpy(np.array(pre, dtype=np.float32)).to(dtype), 0).permute(0, 3, 1, 2)


def stored_modules(rec):
    """The per-module tensors the fixtures keep: every child of the network, each block's two first batch norms (the branches
    the GPU stores), and the _upsample_add results."""
    return [k for k in rec if k not in ("final", "preclamp") and (k.count(".") == 0 or k.endswith((".res_bn", ".bn1")))]


def record():
    """-> {key: array}: everything the fixtures hold (float64 where the fixtures keep float64, float32 otherwise)."""
    assert available(), "the reference tree is not mounted"
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one summation order, whatever the machine offers
    try:
        return _record()
    finally:
        torch.set_num_threads(threads)


def _record():
    sd, wsha = weights()
    m64, m32 = reference_model(sd, torch.float64), reference_model(sd, torch.float32)
    test_new = reference_function("train.py", "test", {"torch": torch})
    test_old = reference_function("train.py", "test", {"torch": _OldTorch()})
    get_score = reference_function("load_data.py", "get_score", {"np": np})
    data = {"meta/seed": np.int64(SEED), "meta/sizes": np.array(SIZES, np.int64), "meta/sha_weights": np.array(wsha)}
    differ, agree, clamped, total, apart = 0, 0, 0, 0, 0.0
    for (w, h), frame in inputs().items():
        s = tag(w, h)
        data[f"{s}/input"] = frame
        data[f"meta/sha_{s}"] = np.array(sha256(frame.tobytes()))
        # train.py:test(), both readings of torch.max
        pre_old, rgb_old = run_test(test_old, m32, frame, aligned=True)
        pre_new, rgb_new = run_test(test_new, m32, frame, aligned=False)
        mx = frame[..., 9:14].reshape(-1, 5).max(0)
        div_old = np.array([np.float32(KEPS + float(v)) for v in mx], np.float32)
        div_new = (np.float32(KEPS) + mx).astype(np.float32)
        delta = pre_new.view(np.int32).astype(np.int64) - pre_old.view(np.int32).astype(np.int64)
        assert np.abs(delta).max() <= 127
        same = div_old == div_new
        differ += int(not same.all())
        agree += int(same.all())
        data[f"{s}/pre_v02"], data[f"{s}/pre_installed_delta"] = pre_old, delta.astype(np.int8)
        data[f"{s}/div_v02"], data[f"{s}/div_installed"] = div_old, div_new
        data[f"{s}/test_rgb_v02"], data[f"{s}/test_rgb_installed"] = rgb_old, rgb_new
        # the network, three ways, on the 0.2/0.3 pre-processing
        runs = {"aligned": run_network(m64, nchw(pre_old, torch.float64), True),
                "installed": run_network(m64, nchw(pre_old, torch.float64), False),
                "f32": run_network(m32, nchw(pre_old, torch.float32), True)}
        assert np.array_equal(runs["f32"]["final"][0].permute(1, 2, 0).numpy(), rgb_old)  # test() is that run
        ali, ins = runs["aligned"], runs["installed"]
        e32 = {k: float((runs["f32"][k].double() - ali[k]).abs().max()) for k in ali}
        data[f"{s}/e32_names"], data[f"{s}/e32_values"] = np.array(list(e32)), np.array(list(e32.values()), np.float64)
        for run in ("aligned", "installed"):
            for k in ("final", "preclamp"):
                data[f"{s}/{run}/{k}"] = runs[run][k][0].numpy().copy()
        if (w, h) in PER_MODULE:
            for k in stored_modules(ali):
                data[f"{s}/aligned/{k}"] = ali[k][0].numpy().astype(np.float32)
                if not torch.equal(ali[k], ins[k]):
                    data[f"{s}/installed/{k}"] = ins[k][0].numpy().astype(np.float32)
        # the pre-clamp tensor is the head times (0.00316 + albedo), and the result is its clamp
        x64 = nchw(pre_old, torch.float64)
        assert torch.equal(ali["preclamp"], ali["rgb_conv"] * (KEPS + x64[:, 6:9]))
        assert torch.equal(ali["final"], ali["preclamp"].clamp(0, 1))
        fin, pc = ali["final"], ali["preclamp"]
        margin = torch.minimum(pc.abs(), (pc - 1).abs())[(pc < 0) | (pc > 1)]
        # a clamped value lies further from the clamp than the GPU tests' bound on the result, so that code which meets
        # the bound must give exactly 0 or 1 there
        assert margin.numel() == 0 or margin.min() > 8 * e32["final"] + 4 * 2.0 ** -23, (s, float(margin.min()))
        clamped += int(((fin <= 0) | (fin >= 1)).sum())
        total += fin.numel()
        apart = max(apart, float((ali["final"] - ins["final"]).abs().max()))
        # load_data.py:get_score, on the frame as the reference lays it out: float64 [14][W][H]
        laid = np.swapaxes(pre_old.astype(np.float64), 0, 2)
        for p in SCORE_PATCHES:
            if p <= min(w, h):
                cs = corners(w, h, p)
                data[f"{s}/score_corners_P{p}"] = np.array(cs, np.int64)
                data[f"{s}/score_P{p}"] = np.array([get_score(laid[:, x:x + p, y:y + p]) for x, y in cs], np.float64)
    assert differ >= 1, "no input has a divisor that differs between the two readings of torch.max"
    assert agree >= 1, "no input has equal divisors under both readings of torch.max"
    assert apart > 0.1, f"installed and aligned upsampling differ by {apart} only"
    assert 2 * clamped < total, f"{clamped} of {total} final outputs are clamped"
    return data


# ---- files ------------------------------------------------------------------------------------------------------------------

def write(data, out_dir):
    """Write `data` as ref_denoise_<group>_<n>.npz files of at most LIMIT bytes each; an array too large for one file is cut
    into flat parts "key#i" with its shape under "key#shape" (tests/denoise_reference_fixture.py puts them together)."""
    os.makedirs(out_dir, exist_ok=True)
    for name in os.listdir(out_dir):
        if name.startswith(PREFIX) and name.endswith(".npz"):
            os.remove(os.path.join(out_dir, name))
    groups = {}
    for key in sorted(data):
        a = np.asarray(data[key])
        g = groups.setdefault(key.split("/")[0], [])
        if a.nbytes <= CHUNK:
            g.append((key, a))
        else:
            flat = np.ascontiguousarray(a).ravel()
            per = CHUNK // a.itemsize
            g.append((key + "#shape", np.array(a.shape, np.int64)))
            for i in range(0, flat.size, per):
                g.append((f"{key}#{i // per}", flat[i:i + per]))
    written = []
    for group, items in groups.items():
        files, cur, size = [], {}, 0
        for key, a in items:
            if cur and size + a.nbytes > CHUNK:
                files.append(cur)
                cur, size = {}, 0
            cur[key] = a
            size += a.nbytes
        files.append(cur)
        for n, cur in enumerate(files):
            path = os.path.join(out_dir, f"{PREFIX}{group}_{n}.npz")
            np.savez_compressed(path, **cur)
            assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
            written.append(path)
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    paths = write(record(), args.out)
    total = sum(os.path.getsize(p) for p in paths)
    print(f"ref_denoise: {len(paths)} files, {total} bytes, largest {max(os.path.getsize(p) for p in paths)} -> {args.out}")


if __name__ == "__main__":
    main()
