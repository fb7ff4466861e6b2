#!/usr/bin/env python3
"""Times the training-patch stage (pt_patches_*, csrc/pt_patches.hip) against the same three steps written in torch on the same
device, the path a user would take without the stage: amax of channels 9-13 (prepare); the colour's division, slicing and var in
float64 of colour and normal per candidate (score); both divisions, slicing, permute and stack (gather).  A comparison point,
not a bar: the torch path computes the reference's float64 measure, not this stage's exact sums.  Arms alternate inside one
process, as in tools/compare_times.py: a window is --calls back-to-back asynchronous calls of one arm, closed by a device
synchronise, under a host clock; the time of a window is divided by its calls.  Per arm: the median, minimum and maximum over
--windows windows after --warmup windows of every arm.  The gather's achieved bytes per second are the bytes it must move,
N P P (56 + 4 stride read, 68 written), over its median time.

  python3 tools/patches_times.py [--size 512] [--patch 256] [--candidates 64] [--patches 16] [--windows 30] [--calls 50]
                                 [--warmup 3] [--no-torch] [--out DIR]
      -> patches_times.json
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def pair_of(size, seed=1):
    rng = np.random.default_rng(seed)
    base = np.exp(rng.normal(-1.0, 1.5, (size, size, 3)))
    f = np.empty((size, size, 14), np.float32)
    f[..., 0:3] = base * np.exp(rng.normal(0.0, 0.5, base.shape))
    f[..., 3:6] = rng.uniform(-1.0, 1.0, (size, size, 3))
    f[..., 6:9] = rng.uniform(0.0, 1.0, (size, size, 3))
    f[..., 9] = rng.uniform(0.0, 300.0, (size, size))
    f[..., 10:14] = np.exp(rng.normal(-2.0, 1.0, (size, size, 4)))
    g = rng.standard_normal((size, size, 14)).astype(np.float32)
    g[..., :3] = base
    return f, g


def windows(pt, arms, n_windows, calls, warmup):
    """arms: {name: callable that enqueues one call}.  -> {name: seconds per call, one entry per window}."""
    out = {k: [] for k in arms}
    for w in range(warmup + n_windows):
        for name, call in arms.items():  # (alternating: every arm sees the same drift)
            pt.check(pt.lib.pt_device_synchronize())
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            pt.check(pt.lib.pt_device_synchronize())
            if w >= warmup:
                out[name].append((time.perf_counter() - t0) / calls)
    return out


def summary(samples):
    a = np.array(samples) * 1e6
    return {"median_us": round(float(np.median(a)), 3), "min_us": round(float(a.min()), 3), "max_us": round(float(a.max()), 3)}


def torch_arms(frame, gt, p, candidates, chosen):
    """The same three steps in torch on the device; every arm leaves its result on the device."""
    import torch

    dev = torch.device("cuda:0")
    t, g = torch.from_numpy(frame).to(dev), torch.from_numpy(gt).to(dev)
    eps = 0.00316
    keep = {}

    def prepare():
        keep["div"] = eps + t[..., 9:14].amax(dim=(0, 1))

    def score():
        colour = t[..., 0:3] / (eps + t[..., 6:9])
        out = []
        for x, y in candidates:
            c, n = colour[y:y + p, x:x + p].double(), t[y:y + p, x:x + p, 3:6].double()
            out.append(c.var(unbiased=False) + n.var(unbiased=False))
        keep["scores"] = torch.stack(out)

    def gather():
        pre = torch.cat([t[..., 0:3] / (eps + t[..., 6:9]), t[..., 3:9], t[..., 9:14] / keep["div"]], dim=-1)
        keep["inputs"] = torch.stack([pre[y:y + p, x:x + p].permute(2, 0, 1) for x, y in chosen]).contiguous()
        keep["targets"] = torch.stack([g[y:y + p, x:x + p, 0:3].clamp(0.0, 1.0).permute(2, 0, 1) for x, y in chosen]).contiguous()

    prepare()
    return {"torch_prepare": prepare, "torch_score": score, "torch_gather": gather}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--patches", type=int, default=16)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches"))
    args = ap.parse_args()
    if not args.no_torch:  # (torch first, as in bench.py: both then share the HIP runtime that torch brings up)
        import torch

        if not torch.cuda.is_available():
            sys.exit("patches_times.py: torch sees no GPU (--no-torch times the stage alone)")
        torch.cuda.set_device(0)
    pt = ge.load_package()
    try:
        devices = pt.device_count()
    except pt.PtError:
        devices = 0
    if devices < 1:
        sys.exit("patches_times.py: no HIP device (there is nothing to time on a CPU)")
    pt.set_device(0)
    size, p, nc, n = args.size, args.patch, args.candidates, args.patches
    frame, gt = pair_of(size)
    rng = random.Random(1)
    candidates = [(rng.randint(0, size - p), rng.randint(0, size - p)) for _ in range(nc)]
    chosen = candidates[:n]
    ps = pt.Patches(size, size, p, max_patches=nc)
    d_train, d_gt = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(gt.nbytes).upload(gt)
    d_in, d_t = pt.DeviceBuffer(n * 14 * p * p * 4), pt.DeviceBuffer(n * 3 * p * p * 4)
    result = {"fingerprint": pt.build_fingerprint(), "device": pt.device_info(), "size": size, "patch": p, "candidates": nc, "patches": n,
              "windows": args.windows, "calls": args.calls, "warmup": args.warmup}
    try:
        ps.run_prepare(d_train.ptr)
        arms = {
            "prepare": lambda: ps.prepare(d_train.ptr),
            "score": lambda: ps.enqueue_score(d_train.ptr, candidates),
            "gather": lambda: ps.enqueue_gather(d_train.ptr, chosen, d_in.ptr, d_gt=d_gt.ptr, d_targets=d_t.ptr),
        }
        keep = None
        if not args.no_torch:
            extra, keep = torch_arms(frame, gt, p, candidates, chosen)
            arms.update(extra)
        t = windows(pt, arms, args.windows, args.calls, args.warmup)
        result["arms"] = {k: summary(v) for k, v in t.items()}
        moved = n * p * p * (56 + 4 * 14 + 68)
        result["gather_bytes"] = moved
        result["gather_gb_per_s"] = round(moved / (result["arms"]["gather"]["median_us"] * 1e-6) / 1e9, 1)
        result["score_first"] = ps.result(0)["score"]
        result["workspace_bytes"] = ps.memory()["workspace"]
        if keep is not None:
            for k in ("prepare", "score", "gather"):
                result[f"torch_over_{k}"] = round(result["arms"][f"torch_{k}"]["median_us"] / result["arms"][k]["median_us"], 2)
            got = d_in.download(np.float32, (n, 14, p, p))
            result["max_abs_difference_from_torch_inputs"] = float(np.nanmax(np.abs(got - keep["inputs"].cpu().numpy())))
            result["torch_score_first"] = float(keep["scores"][0].item())
    finally:
        ps.destroy()
        for d in (d_train, d_gt, d_in, d_t):
            d.free()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "patches_times.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
