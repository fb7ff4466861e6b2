#!/usr/bin/env python3
"""Times the feature-guided filter (pt_filter_*, csrc/pt_filter.hip) with device events on rendered Cornell frames: warm-up,
then the median of --runs windows per case.  Every run is out of place (the frames stay as rendered, so every window filters
the same data).  Each case is timed three times: the product library as shipped, and the lab library (the same kernels) with
steps 1 and 2 forced to direct loads and to the LDS tile (pt_debug_filter_tiled) -- the A/B behind DENOISER.md's decision.
Beside it, in the same session, the CNN's fp32 single-frame time (pt_denoiser_denoise, random weights).

  python3 tools/filter_time.py [--cases 128:1 512:1 1024:1 128:32 512:32] [--runs 100] [--warmup 10] [--no-cnn] [--out DIR]
      case = SIZE:FRAMES; FRAMES > 1 goes through pt_filter_run_frames with max_frames = FRAMES -> filter_time.json
  python3 tools/filter_time.py --trace-run SIZE [--frames N] [--tiled on|off]
      the workload for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/filter_time.py --trace-run SIZE`
  python3 tools/filter_time.py --trace DIR|FILE --size SIZE [--frames N] [--label NAME] [--out DIR]
      per-iteration kernel times from that trace -> iterations_SIZE[_nN][_NAME].txt, with each iteration's achieved bytes/s against
      the kernel's own load count: 25 taps x 48 B + 9 x 4 B per pixel (what the lanes ask for, from the caches or from the LDS tile)
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SPP = 4
TAP_BYTES = 25 * 48 + 9 * 4  # loads one pixel issues per iteration
PREPARE_BYTES = 14 * 4 + 4 * 4 + 48  # frame pixel + four depth neighbours read, three float4 written


def frames_of(pt, size, n):
    out = []
    for k in range(n):
        eye = (50.0 + 0.7 * (k % 8), 52.0 - 0.3 * (k % 8), 295.6 - 1.1 * (k % 8))
        basis = pt.camera_basis(eye, yaw=-90.0 + 0.9 * (k % 8), pitch=-0.4 * (k % 8), width=size, height=size)
        out.append(pt.render_frame(size, size, SPP, basis=basis, eye=eye)[0] if k < 8 else out[k % 8])
    return np.stack(out)


def time_filter(pt, size, n, runs, warmup, tiled=None):
    """Device-event ms (pt_filter_run / pt_filter_run_frames) of `runs` windows after `warmup`.  tiled: None = as the library
    decides, True / False = steps 1 and 2 with / without the LDS tile (lab library)."""
    frames = frames_of(pt, size, n)
    ff = pt.FeatureFilter(size, size, max_frames=n)
    if tiled is not None:
        ff.tiled(tiled)
    d_frames = pt.DeviceBuffer(frames.nbytes).upload(frames)
    d_rgb = pt.DeviceBuffer(n * size * size * 12)
    try:
        t = []
        for i in range(warmup + runs):
            ms = ff.run(d_frames.ptr, SPP, d_rgb.ptr) if n == 1 else ff.run_frames(d_frames.ptr, n, SPP, d_rgb=d_rgb.ptr)
            if i >= warmup:
                t.append(ms)
        mem = ff.memory()
    finally:
        d_frames.free()
        d_rgb.free()
        ff.destroy()
    return np.array(t), mem


def time_cnn(pt, size, runs, warmup):
    from cuda_pathtrace_amd import denoise_weights as dw

    frame = frames_of(pt, size, 1)[0]
    dn = pt.Denoiser(size, size, dw.random_state_dict(seed=1))
    d_frame = pt.DeviceBuffer(frame.nbytes).upload(frame)
    d_rgb = pt.DeviceBuffer(size * size * 12)
    try:
        t = []
        for i in range(warmup + runs):
            ms = dn.denoise(d_frame.ptr, d_rgb.ptr)
            if i >= warmup:
                t.append(ms)
    finally:
        d_frame.free()
        d_rgb.free()
        dn.destroy()
    return np.array(t)


def from_trace(path):
    """[(kernel name, start ns, end ns)] of the filter's kernels in launch order, from a kernel_trace.csv."""
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[-1]
    with open(path) as f:
        recs = list(csv.DictReader(f))
    key_name = next(k for k in recs[0] if k.lower() in ("kernel_name", "kernelname"))
    key_s = next(k for k in recs[0] if k.lower() in ("start_timestamp", "begin_ns", "start"))
    key_e = next(k for k in recs[0] if k.lower() in ("end_timestamp", "end_ns", "end"))
    recs = [(r[key_name], int(r[key_s]), int(r[key_e])) for r in recs if "ptflt" in r[key_name]]
    recs.sort(key=lambda r: r[1])
    return path, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["128:1", "512:1", "1024:1", "128:32", "512:32"])
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-cnn", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", type=int, default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--tiled", choices=["on", "off"], default=None, help="--trace-run: force the LDS tile of steps 1 and 2 (lab library)")
    ap.add_argument("--label", default="", help="--trace: suffix of the table's file name")
    a = ap.parse_args()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.trace:
        path, recs = from_trace(a.trace)
        per = 1 + a.iterations
        groups = len(recs) // per
        assert groups >= 4 and all("prepare" in recs[g * per][0] for g in range(groups)), (len(recs), per)
        px = a.size * a.size * a.frames
        names = ["prepare"] + [f"iteration {i} (step {1 << i})" + (", fused store" if i == a.iterations - 1 else "") for i in range(a.iterations)]
        lines = [f"per-kernel times at {a.size}x{a.size}, {a.frames} frame(s) per launch, median over the last {groups - 2} of {groups} "
                 f"filter runs of {os.path.basename(path)}",
                 f"{'kernel':36s} {'us':>9s} {'requested MB':>13s} {'GB/s':>8s}"]
        total = 0.0
        for k, name in enumerate(names):
            us = float(np.median([(recs[g * per + k][2] - recs[g * per + k][1]) * 1e-3 for g in range(2, groups)]))
            mb = px * (PREPARE_BYTES if k == 0 else TAP_BYTES + (12 if k == a.iterations else 16)) / 1e6
            total += us
            lines.append(f"{name:36s} {us:9.2f} {mb:13.2f} {mb / us * 1e3:8.0f}")
        lines.append(f"{'sum of kernels':36s} {total:9.2f}")
        text = "\n".join(lines)
        print(text)
        if a.out:
            name = f"iterations_{a.size}" + (f"_n{a.frames}" if a.frames > 1 else "") + (f"_{a.label}" if a.label else "") + ".txt"
            open(os.path.join(a.out, name), "w").write(text + "\n")
        return
    pt = ge.load_package()
    lab = ge.load_lab()  # the same kernels, plus the switch between the direct and the tiled form of steps 1 and 2
    pt.set_device(0)
    if a.trace_run:
        t, _ = time_filter(lab if a.tiled else pt, a.trace_run, a.frames, 20, 2, None if a.tiled is None else a.tiled == "on")
        print(f"{a.trace_run}x{a.trace_run} n={a.frames} tiled={a.tiled}: median {np.median(t):.4f} ms under the tracer")
        return
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
           "frame": f"Cornell box, {SPP} spp, up to 8 poses", "options": "defaults (5 iterations)",
           "note": "ms_per_frame = median device-event window of one call / n; out of place", "filter": {}, "filter_lab_direct": {}, "filter_lab_tiled": {}, "cnn_fp32": {}}
    for case in a.cases:
        size, n = (int(v) for v in case.split(":"))
        # the product library as shipped, then the lab library with steps 1 and 2 forced each way
        for key, mod, tiled in (("filter", pt, None), ("filter_lab_direct", lab, False), ("filter_lab_tiled", lab, True)):
            t, mem = time_filter(mod, size, n, a.runs, a.warmup, tiled)
            e = {"call_ms_median": float(np.median(t)), "call_ms_min": float(t.min()), "call_ms_max": float(t.max()),
                 "ms_per_frame": float(np.median(t)) / n, "workspace_bytes": mem["workspace"]}
            res[key][case] = e
            print(f"{key} {size}x{size} n={n}: call {e['call_ms_median']:.4f} ms (min {e['call_ms_min']:.4f}), {e['ms_per_frame']:.4f} ms per "
                  f"frame, workspace {mem['workspace'] / 1e6:.1f} MB", flush=True)
    if not a.no_cnn:
        for size in sorted({int(c.split(":")[0]) for c in a.cases}):
            t = time_cnn(pt, size, max(a.runs // 4, 20), 5)
            res["cnn_fp32"][str(size)] = {"ms_median": float(np.median(t)), "ms_min": float(t.min())}
            print(f"cnn fp32 {size}x{size} n=1: {np.median(t):.4f} ms", flush=True)
    if a.out:
        with open(os.path.join(a.out, "filter_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
