#!/usr/bin/env python3
"""Times the feature filter's spatial variance estimate (pt_filter_set_spatial; spatial_kernel of csrc/pt_filter.hip) with device
events on rendered 1-spp Cornell frames, a sibling of tools/filter_time.py.

  python3 tools/filter_spatial_time.py [--sizes 512 1024] [--runs 200] [--warmup 20] [--processes 5] [--parent-lib FILE] [--out DIR]
      Starts --processes fresh child processes one after the other.  Each child times, per size, pt_filter_run (5 iterations,
      out of place) with the mode off, with it on for every pixel at R = 1, 2, 3 and, with --parent-lib (a libptcore.so built
      from the parent commit, loaded beside this build's in the same process), the parent's filter: the cases alternate window
      by window, so drift of the machine hits all alike.  Reported: the median over the children of each child's median
      window, the spread of those medians, and on - off.  "off" and "parent" issue identical launches.
      -> filter_spatial_time.json
  python3 tools/filter_spatial_time.py --child ...      one such process; prints one JSON line
      Under `rocprofv3 --kernel-trace --stats -- python3 tools/filter_spatial_time.py --child --runs 20` the per-kernel
      averages give spatial_kernel<R> beside the iterations.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = 1
CASES = ("off", "on[1]", "on[2]", "on[3]")


def child(a):
    import __graft_entry__ as ge

    pt = ge.load_package()
    pt.set_device(0)
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("pt_filter_create", "pt_filter_run", "pt_filter_destroy"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = pt.ABI[name]
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "cases": {}}
    for size in a.sizes:
        frame = pt.render_frame(size, size, SPP, basis=pt.camera_basis(width=size, height=size))[0]
        d_frame, d_rgb = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(size * size * 12)
        filters = {"off": pt.FeatureFilter(size, size)}
        for R in (1, 2, 3):
            filters[f"on[{R}]"] = pt.FeatureFilter(size, size, spatial_below="all", spatial_radius=R)
        runs = {k: (lambda f=f: f.run(d_frame.ptr, SPP, d_rgb.ptr)) for k, f in filters.items()}
        handle = ctypes.c_void_p()
        if parent:
            pt.check(parent.pt_filter_create(size, size, None, ctypes.byref(handle)))
            ms = ctypes.c_float()

            def run_parent():
                pt.check(parent.pt_filter_run(handle, d_frame.ptr, d_rgb.ptr, SPP, None, ctypes.byref(ms)))
                return ms.value
            runs["parent"] = run_parent
        try:
            t = {k: [] for k in runs}
            for i in range(a.warmup + a.runs):
                for k, run in runs.items():  # alternating, window by window
                    v = run()
                    if i >= a.warmup:
                        t[k].append(v)
            res["cases"][str(size)] = {k: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v))} for k, v in t.items()}
        finally:
            for f in filters.values():
                f.destroy()
            if parent:
                parent.pt_filter_destroy(handle)
            d_frame.free()
            d_rgb.free()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[512, 1024])
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--runs", str(a.runs), "--warmup", str(a.warmup), "--sizes"] + [str(s) for s in a.sizes]
    if a.parent_lib:
        cmd += ["--parent-lib", a.parent_lib]
    children = []
    for k in range(a.processes):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit(f"child {k} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
        children.append(json.loads(next(line for line in out.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    res = {"device": children[0]["device"], "fingerprint": children[0]["fingerprint"], "processes": a.processes, "runs": a.runs,
           "warmup": a.warmup, "frame": f"Cornell box, default camera, {SPP} spp; 5 iterations, out of place, below = all",
           "note": "ms = median over the processes of each process's median device-event window of pt_filter_run; the cases "
                   "alternate window by window inside a process", "cases": {}}
    for size in (str(s) for s in a.sizes):
        e = res["cases"][size] = {}
        for k in children[0]["cases"][size]:
            med = [c["cases"][size][k]["ms_median"] for c in children]
            e[k] = {"ms": float(np.median(med)), "ms_lowest_process": float(min(med)), "ms_highest_process": float(max(med)),
                    "ms_min_window": float(min(c["cases"][size][k]["ms_min"] for c in children))}
        for R in (1, 2, 3):
            e[f"on[{R}]"]["extra_ms"] = e[f"on[{R}]"]["ms"] - e["off"]["ms"]
        line = f"{size}x{size}: " + ", ".join(f"{k} {v['ms']:.4f} ms [{v['ms_lowest_process']:.4f} .. {v['ms_highest_process']:.4f}]" for k, v in e.items())
        print(line, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "filter_spatial_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
