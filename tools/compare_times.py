#!/usr/bin/env python3
"""Times the comparison stage (pt_compare_*, csrc/pt_compare.hip) against the tone mapper with a metered exposure
(pt_tonemap_enqueue, three launches), the nearest yardstick the project has: one pass with a reduction over ONE input, where the
comparison reads two.  Arms alternate inside one process, as in tools/tonemap_times.py: a window is --calls back-to-back
asynchronous calls of one arm, closed by a device synchronise, under a host clock; the time of a window is divided by its calls.
Per arm: the median, minimum and maximum over --windows windows after --warmup windows of every arm.

  python3 tools/compare_times.py [--sizes 512 2048] [--batch 32] [--windows 50] [--calls 200] [--warmup 5] [--out DIR]
      arms per size: tonemap (auto), compare (no map), compare_map; then the same three over --batch frames of that size in one
      call (max_frames = --batch, or what 2^26 pixels per group allow), per frame.  The image is a frame (pixel stride 14), the reference an rgb image (stride 3),
      as the command-line front end compares them; the frames of a batch are copies of one frame at different addresses.
      -> compare_times.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def pair_of(size, seed=1):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((size, size, 14)).astype(np.float32)
    ref = np.exp2(rng.uniform(-8.0, 4.0, (size, size, 3))).astype(np.float32)
    f[..., :3] = ref * np.exp(rng.normal(0.0, 0.5, ref.shape)).astype(np.float32)
    return f, ref


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


def summary(samples, per=1):
    a = np.array(samples) * 1e6 / per
    return {"median_us": round(float(np.median(a)), 3), "min_us": round(float(a.min()), 3), "max_us": round(float(a.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare"))
    args = ap.parse_args()
    pt = ge.load_package()
    try:
        devices = pt.device_count()
    except pt.PtError:
        devices = 0
    if devices < 1:
        sys.exit("compare_times.py: no HIP device (there is nothing to time on a CPU)")
    pt.set_device(0)
    result = {"fingerprint": pt.build_fingerprint(), "device": pt.device_info(), "windows": args.windows, "calls": args.calls,
              "warmup": args.warmup, "cases": {}}
    n = args.batch
    for size in args.sizes:
        frame, ref = pair_of(size)
        px = size * size
        d_img, d_ref = pt.DeviceBuffer(n * frame.nbytes), pt.DeviceBuffer(n * ref.nbytes)
        for k in range(n):  # n copies of the pair, each at its own address
            pt.check(pt.lib.pt_memcpy_h2d(d_img.ptr + k * frame.nbytes, frame.ctypes.data, frame.nbytes))
            pt.check(pt.lib.pt_memcpy_h2d(d_ref.ptr + k * ref.nbytes, ref.ctypes.data, ref.nbytes))
        d_map, d_rgba = pt.DeviceBuffer(n * px * 12), pt.DeviceBuffer(n * px * 4)
        group = max(1, min(n, (1 << 26) // px))  # (the stages' limit of 2^26 pixels per group: 32 at 512^2, 16 at 2048^2)
        one, many = pt.Compare(size, size), pt.Compare(size, size, max_frames=group)
        tone, tones = pt.Tonemap(size, size, adapt=0.5), pt.Tonemap(size, size, adapt=0.5, max_frames=group)
        try:
            arms = {
                "tonemap": lambda: tone.enqueue(d_img.ptr, d_rgba.ptr),
                "compare": lambda: one.enqueue(d_img.ptr, d_ref.ptr, None, ref_pixel_stride=3),
                "compare_map": lambda: one.enqueue(d_img.ptr, d_ref.ptr, d_map.ptr, ref_pixel_stride=3),
            }
            t = windows(pt, arms, args.windows, args.calls, args.warmup)
            case = {k: summary(v) for k, v in t.items()}
            case["compare_over_tonemap"] = round(case["compare"]["median_us"] / case["tonemap"]["median_us"], 3)
            result["cases"][f"{size}"] = case
            values = one.result(0)
            result["cases"][f"{size}"]["values"] = {k: values[k] for k in ("rms", "relmse", "ssim", "saturated")}
            arms = {
                "tonemap": lambda: tones.enqueue_frames(d_img.ptr, n, d_rgba.ptr),
                "compare": lambda: many.enqueue_frames(d_img.ptr, n, d_ref.ptr, None, ref_pixel_stride=3),
                "compare_map": lambda: many.enqueue_frames(d_img.ptr, n, d_ref.ptr, d_map.ptr, ref_pixel_stride=3),
            }
            t = windows(pt, arms, args.windows, max(1, args.calls // n), args.warmup)
            case = {k + "_per_frame": summary(v, per=n) for k, v in t.items()}
            case["compare_over_tonemap"] = round(case["compare_per_frame"]["median_us"] / case["tonemap_per_frame"]["median_us"], 3)
            case["max_frames"] = group
            result["cases"][f"{n}x{size}"] = case
        finally:
            for s in (one, many, tone, tones):
                s.destroy()
            for d in (d_img, d_ref, d_map, d_rgba):
                d.free()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "compare_times.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["cases"], indent=1))


if __name__ == "__main__":
    main()
