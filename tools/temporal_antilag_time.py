#!/usr/bin/env python3
"""Times the responsive history of the temporal accumulator (pt_temporal_set_antilag; the FAST accumulate launch and
rectify_kernel of csrc/pt_temporal.hip) with device events on rendered Cornell frames, a sibling of tools/temporal_motion_time.py.

  python3 tools/temporal_antilag_time.py [--sizes 512 1024] [--runs 60] [--warmup 10] [--fast-cap 8] [--out DIR]
      per size the median window of pt_temporal_run for
        static     anti-lag off: the static accumulate launch
        whole[R]   anti-lag on, clamp_radius R = 1, 2, 3: the FAST accumulate launch + rectify_kernel<R>
      A session offers no window around one of its two launches, so the split is taken from a kernel trace of this same
      program: run it under `rocprofv3 --kernel-trace --stats -- python3 tools/temporal_antilag_time.py --runs 20` and read the
      per-kernel averages (accumulate_kernel<false, const float4*, float4*, float>, rectify_kernel<R>) per grid size.
      -> temporal_antilag_time.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import __graft_entry__ as ge  # noqa: E402
import temporal_motion_time as tmt  # noqa: E402

SPP = tmt.SPP


def time_size(pt, size, runs, warmup, fast_cap):
    frames, _, basis = tmt.two_frames(pt, size)
    d_frame, d_counts = pt.DeviceBuffer(frames[0].nbytes), pt.DeviceBuffer(size * size * 4)
    res = {}
    try:
        for name, opts in [("static", {})] + [(f"whole[{R}]", dict(fast_cap=fast_cap, clamp_radius=R)) for R in (1, 2, 3)]:
            ta = pt.Temporal(size, size, **opts)
            try:
                res[name + "_ms"], res[name + "_ms_min"] = tmt.median_window(
                    lambda k: ta.run(d_frame.ptr, SPP, basis, d_counts=d_counts.ptr), frames, d_frame, runs, warmup)
                res[name + "_per_pixel_bytes"] = ta.memory()["per_pixel"]
            finally:
                ta.destroy()
    finally:
        d_frame.free()
        d_counts.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[512, 1024])
    ap.add_argument("--runs", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fast-cap", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pt = ge.load_package()
    pt.set_device(0)
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
           "fast_cap": a.fast_cap, "frame": f"Cornell box, {SPP} spp, sphere 7 moved between two frames", "cases": {}}
    for size in a.sizes:
        e = res["cases"][str(size)] = time_size(pt, size, a.runs, a.warmup, a.fast_cap)
        print(f"{size}x{size}: static {e['static_ms']:.4f} ms; anti-lag whole call R=1 {e['whole[1]_ms']:.4f}, R=2 {e['whole[2]_ms']:.4f}, "
              f"R=3 {e['whole[3]_ms']:.4f} ms", flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "temporal_antilag_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
