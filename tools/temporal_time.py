#!/usr/bin/env python3
"""Times the temporal accumulator (pt_temporal_*, csrc/pt_temporal.hip) with device events on rendered Cornell frames of a
fly-through: warm-up, then the median of --runs windows per case.  A window is one pt_temporal_run (FRAMES = 1) or one
pt_temporal_run_frames over FRAMES frames with a count image; the frames are uploaded again before every window (outside it), the
history carries on from window to window, so every launch of a window gathers.  Each time is also expressed as bytes per
second over the stage's own traffic: 56 + 4 x 48 B read and 16 + 48 + 4 B written per pixel.  Beside it, in the same session,
the feature-guided filter's whole call.

  python3 tools/temporal_time.py [--cases 128:1 512:1 1024:1 128:16 512:16 1024:16] [--runs 100] [--warmup 10] [--out DIR]
      case = SIZE:FRAMES -> temporal_time.json
  python3 tools/temporal_time.py --trace-run SIZE
      the workload for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/temporal_time.py --trace-run SIZE`:
      accumulator and filter alternate, so the trace holds both kernels' times from one session
  python3 tools/temporal_time.py --trace DIR|FILE --size SIZE [--out DIR]
      the accumulator's kernel time from that trace against the yardstick, the filter's set-up kernel (`prepare`: 72 B read
      and 48 B written per pixel) -> kernels_SIZE.txt
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
STAGE_BYTES = (56 + 4 * 48) + (16 + 48 + 4)  # per pixel: the frame pixel and four history taps read; colour + variance, history, count written
PREPARE_BYTES = 14 * 4 + 4 * 4 + 48          # the filter's set-up kernel: frame pixel + four depth neighbours read, three float4 written
POSES = 8


def fly_through(pt, size, n):
    """n rendered frames [n][size][size][14] (8 poses, repeated back and forth), their bases and eyes."""
    order = [j if j < POSES else 2 * POSES - 1 - j for j in (i % (2 * POSES) for i in range(n))]
    poses = [((50.0 + 1.5 * k, 52.0, 295.6 - 2.0 * k), -90.0 + 0.7 * k) for k in range(POSES)]
    bases = [pt.camera_basis(eye, yaw=yaw, width=size, height=size) for eye, yaw in poses]
    r = pt.Renderer(size, size, SPP)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    d_out = pt.DeviceBuffer(size * size * 14 * 4)
    try:
        frames = []
        for k in order:
            r.render(d_out.ptr, d_scene.ptr, ns, bases[k], poses[k][0])
            frames.append(d_out.download(np.float32, (size, size, 14)))
    finally:
        d_out.free()
        d_scene.free()
        r.destroy()
    return np.stack(frames), np.stack([bases[k] for k in order]), np.asarray([poses[k][0] for k in order], dtype=np.float32)


def time_temporal(pt, size, n, runs, warmup):
    frames, bases, eyes = fly_through(pt, size, n)
    ta = pt.Temporal(size, size)
    d_frames, d_counts = pt.DeviceBuffer(frames.nbytes), pt.DeviceBuffer(size * size * 4)
    try:
        t = []
        for i in range(warmup + runs):
            d_frames.upload(frames)
            if n == 1:
                ms = ta.run(d_frames.ptr, SPP, bases[0], eyes[0], d_counts=d_counts.ptr)
            else:
                ms = ta.run_frames(d_frames.ptr, SPP, bases, eyes, d_counts=d_counts.ptr)
            if i >= warmup:
                t.append(ms)
        mem = ta.memory()
        share = float((d_counts.download(np.uint32, (size, size)) > SPP).mean())
    finally:
        d_frames.free()
        d_counts.free()
        ta.destroy()
    return np.array(t), mem, share


def time_filter(pt, size, runs, warmup):
    frame = fly_through(pt, size, 1)[0][0]
    ff = pt.FeatureFilter(size, size)
    d_frame, d_rgb = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(size * size * 12)
    try:
        t = [ff.run(d_frame.ptr, SPP, d_rgb.ptr) for _ in range(warmup + runs)][warmup:]
    finally:
        d_frame.free()
        d_rgb.free()
        ff.destroy()
    return np.array(t)


def trace_run(pt, size, rounds=24):
    frames, bases, eyes = fly_through(pt, size, POSES)
    ta, ff = pt.Temporal(size, size), pt.FeatureFilter(size, size)
    d_frame, d_counts, d_rgb = pt.DeviceBuffer(frames[0].nbytes), pt.DeviceBuffer(size * size * 4), pt.DeviceBuffer(size * size * 12)
    try:
        for i in range(rounds):
            k = i % POSES
            d_frame.upload(frames[k])
            ta.run(d_frame.ptr, SPP, bases[k], eyes[k], d_counts=d_counts.ptr)
            ff.run(d_frame.ptr, SPP, d_rgb.ptr, d_counts=d_counts.ptr)
    finally:
        for b in (d_frame, d_counts, d_rgb):
            b.free()
        ta.destroy()
        ff.destroy()
    print(f"{size}x{size}: {rounds} rounds of accumulate + filter under the tracer")


def from_trace(path):
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[-1]
    with open(path) as f:
        recs = list(csv.DictReader(f))
    key_name = next(k for k in recs[0] if k.lower() in ("kernel_name", "kernelname"))
    key_s = next(k for k in recs[0] if k.lower() in ("start_timestamp", "begin_ns", "start"))
    key_e = next(k for k in recs[0] if k.lower() in ("end_timestamp", "end_ns", "end"))
    recs = sorted(((r[key_name], int(r[key_s]), int(r[key_e])) for r in recs), key=lambda r: r[1])
    return path, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["128:1", "512:1", "1024:1", "128:16", "512:16", "1024:16"])
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", type=int, default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.trace:
        path, recs = from_trace(a.trace)
        px = a.size * a.size
        lines = [f"kernel times at {a.size}x{a.size} from {os.path.basename(path)}: median over all launches but each kernel's first two",
                 f"{'kernel':28s} {'launches':>8s} {'us':>9s} {'B/pixel':>8s} {'GB/s':>8s}"]
        for name, match, nbytes in (("temporal accumulate", lambda s: "pttmp" in s, STAGE_BYTES),
                                    ("filter prepare (yardstick)", lambda s: "ptflt" in s and "prepare" in s, PREPARE_BYTES)):
            us = [(e - s) * 1e-3 for kn, s, e in recs if match(kn)][2:]
            assert len(us) >= 4, (name, len(us))
            med = float(np.median(us))
            lines.append(f"{name:28s} {len(us):8d} {med:9.2f} {nbytes:8d} {px * nbytes / med * 1e-3:8.0f}")
        text = "\n".join(lines)
        print(text)
        if a.out:
            open(os.path.join(a.out, f"kernels_{a.size}.txt"), "w").write(text + "\n")
        return
    pt = ge.load_package()
    pt.set_device(0)
    if a.trace_run:
        trace_run(pt, a.trace_run)
        return
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
           "frame": f"Cornell box, {SPP} spp, fly-through of {POSES} poses back and forth", "options": "defaults",
           "bytes_per_pixel": STAGE_BYTES,
           "note": "ms_per_frame = median device-event window of one call / n; bytes_per_s = width x height x bytes_per_pixel / that; "
                   "history_share = pixels of the last frame with count > n", "temporal": {}, "filter": {}}
    for case in a.cases:
        size, n = (int(v) for v in case.split(":"))
        t, mem, share = time_temporal(pt, size, n, a.runs, a.warmup)
        per = float(np.median(t)) / n
        e = {"call_ms_median": float(np.median(t)), "call_ms_min": float(t.min()), "call_ms_max": float(t.max()), "ms_per_frame": per,
             "bytes_per_s": size * size * STAGE_BYTES / (per * 1e-3), "history_share": share, "workspace_bytes": mem["workspace"]}
        res["temporal"][case] = e
        print(f"temporal {size}x{size} n={n}: call {e['call_ms_median']:.4f} ms (min {e['call_ms_min']:.4f}), {per:.4f} ms per frame, "
              f"{e['bytes_per_s'] / 1e9:.0f} GB/s, history on {share:.3f} of the pixels", flush=True)
    for size in sorted({int(c.split(":")[0]) for c in a.cases}):
        t = time_filter(pt, size, a.runs, a.warmup)
        res["filter"][str(size)] = {"ms_median": float(np.median(t)), "ms_min": float(t.min())}
        print(f"filter {size}x{size} n=1: {np.median(t):.4f} ms", flush=True)
    if a.out:
        with open(os.path.join(a.out, "temporal_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
