#!/usr/bin/env python3
"""Times the tone-mapping stage (pt_tonemap_*, csrc/pt_tonemap.hip) against the display packer (pt_display_pack), which reads
the same 12 of 56 bytes per pixel and writes 12 where the map kernel writes 4.  Arms alternate inside one process: a window is
--calls back-to-back asynchronous calls of one arm on one synthetic frame, closed by a device synchronise, under a host clock;
the time of a window is divided by its calls.  Per arm: the median, minimum and maximum over --windows windows after --warmup
windows of every arm.

  python3 tools/tonemap_times.py [--sizes 512 2048] [--batch 32:512] [--windows 50] [--calls 200] [--warmup 5] [--out DIR]
      arms per size: pack (pt_display_pack), fixed (one launch), auto (three launches); and for --batch FRAMES:SIZE one
      pt_tonemap_enqueue_frames over FRAMES frames, fixed and auto, per frame  -> tonemap_times.json
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


def frame_of(size, frames=1, seed=1):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((frames, size, size, 14)).astype(np.float32)
    f[..., :3] = np.exp2(rng.uniform(-8.0, 4.0, (frames, size, size, 3))).astype(np.float32)
    return f


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
    ap.add_argument("--batch", default="32:512")
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tonemap"))
    args = ap.parse_args()
    pt = ge.load_package()
    try:
        devices = pt.device_count()
    except pt.PtError:
        devices = 0
    if devices < 1:
        sys.exit("tonemap_times.py: no HIP device (there is nothing to time on a CPU)")
    pt.set_device(0)
    result = {"fingerprint": pt.build_fingerprint(), "device": pt.device_info(), "windows": args.windows, "calls": args.calls,
              "warmup": args.warmup, "cases": {}}
    for size in args.sizes:
        frame = frame_of(size)[0]
        d_src, d_out, d_vtx = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(size * size * 4), pt.DeviceBuffer(size * size * 12)
        fixed, auto = pt.Tonemap(size, size, exposure=1.0), pt.Tonemap(size, size, adapt=0.5)
        try:
            arms = {
                "pack": lambda: pt.check(pt.lib.pt_display_pack(d_src.ptr, size, size, d_vtx.ptr, None)),
                "fixed": lambda: fixed.enqueue(d_src.ptr, d_out.ptr),
                "auto": lambda: auto.enqueue(d_src.ptr, d_out.ptr),
            }
            t = windows(pt, arms, args.windows, args.calls, args.warmup)
            result["cases"][f"{size}"] = {k: summary(v) for k, v in t.items()}
        finally:
            fixed.destroy(), auto.destroy()
            d_src.free(), d_out.free(), d_vtx.free()
    if args.batch:
        n, size = (int(x) for x in args.batch.split(":"))
        frames = frame_of(size, n)
        d_src, d_out = pt.DeviceBuffer(frames.nbytes).upload(frames), pt.DeviceBuffer(n * size * size * 4)
        fixed, auto = pt.Tonemap(size, size, exposure=1.0, max_frames=n), pt.Tonemap(size, size, adapt=0.5, max_frames=n)
        try:
            arms = {"fixed": lambda: fixed.enqueue_frames(d_src.ptr, n, d_out.ptr), "auto": lambda: auto.enqueue_frames(d_src.ptr, n, d_out.ptr)}
            t = windows(pt, arms, args.windows, max(1, args.calls // n), args.warmup)
            result["cases"][f"{n}x{size}"] = {k + "_per_frame": summary(v, per=n) for k, v in t.items()}
        finally:
            fixed.destroy(), auto.destroy()
            d_src.free(), d_out.free()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "tonemap_times.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["cases"], indent=1))


if __name__ == "__main__":
    main()
