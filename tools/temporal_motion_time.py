#!/usr/bin/env python3
"""Times the moving-sphere calls of the temporal accumulator (pt_temporal_motion and the _motion / _scene calls,
csrc/pt_temporal.hip) with device events on rendered Cornell frames, a sibling of tools/temporal_time.py.

  python3 tools/temporal_motion_time.py [--sizes 512 1024] [--spheres 9 1000] [--runs 60] [--warmup 10] [--out DIR]
      per size and sphere count, the median window of
        static   pt_temporal_run                     the static accumulate launch
        motion   pt_temporal_run_motion              the MOTION accumulate launch (a motion image made beforehand)
        scene    pt_temporal_run_scene               upload of the spheres + motion kernel + MOTION accumulate launch
      and motion_kernel = scene - motion: the motion kernel with its 32 n byte upload (a difference of two windows, not an
      event pair of its own); beside it motion_call = pt_temporal_motion alone, --runs calls back to back on the host clock.
      The frames are rendered once from the Cornell box; for n != 9 only the motion kernel's scene changes (pt_scene_random,
      CLOSED: every ray hits, so every lane takes the FP64 branch for some spheres of every round -- close to the kernel's
      worst case; an open scene is cheaper).  -> temporal_motion_time.json
  python3 tools/temporal_motion_time.py --parent-lib PATH [--parent-first] [--sizes 512 1024] [--windows 8] [--runs 40] [--out DIR]
      the static pt_temporal_run of this build against another build of the library (the parent commit's libptcore.so), both
      loaded into this process, in alternating windows A B A B ...: per window the median of --runs calls; reported are the
      median of the windows' medians for each build and the spread (max - min) of the parent's own windows.
      --parent-first creates the parent's session before this build's (the other placement of the two histories in memory).
      -> static_vs_parent.json / static_vs_parent_first.json
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SPP = 4


def load_other(path):
    """The package's ctypes view bound to another build of the library (as __graft_entry__.load_lab does)."""
    spec = importlib.util.spec_from_file_location("cuda_pathtrace_amd_other", os.path.join(ge.PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[ge.PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    old = os.environ.get("PT_LIB_OVERRIDE")
    os.environ["PT_LIB_OVERRIDE"] = os.path.abspath(path)
    try:
        sys.modules["cuda_pathtrace_amd_other"] = mod
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["PT_LIB_OVERRIDE"]
        else:
            os.environ["PT_LIB_OVERRIDE"] = old
    return mod


def two_frames(pt, size):
    """Two rendered frames of the Cornell box with sphere 7 moved by (2.5, 0, 1) in between, their scenes, basis and eye."""
    scenes = [pt.scene_cornell(), pt.scene_cornell()]
    scenes[1]["pos"][7] += np.array([2.5, 0.0, 1.0], np.float32)
    basis = pt.camera_basis(width=size, height=size)
    r = pt.Renderer(size, size, SPP)
    d_scene, ns = pt.upload_scene(scenes[0])
    d_out = pt.DeviceBuffer(size * size * 14 * 4)
    try:
        frames = []
        for s in scenes:
            d_scene.upload(s)
            r.render(d_out.ptr, d_scene.ptr, ns, basis, pt.DEFAULT_EYE)
            frames.append(d_out.download(np.float32, (size, size, 14)))
    finally:
        d_out.free()
        d_scene.free()
        r.destroy()
    return frames, scenes, basis


def median_window(call, frames, d_frame, runs, warmup):
    """Median device-event milliseconds of call(k) over `runs` calls; the frame is uploaded again before every call."""
    t = []
    for i in range(warmup + runs):
        d_frame.upload(frames[i % 2])
        ms = call(i % 2)
        if i >= warmup:
            t.append(ms)
    return float(np.median(t)), float(np.min(t))


def time_motion(pt, size, n, runs, warmup):
    frames, scenes, basis = two_frames(pt, size)
    if n != 9:
        a = pt.scene_random(n, 1, True)
        b = a.copy()
        b["pos"][n // 2:] += np.array([0.5, 0.0, 0.25], np.float32)
        scenes = [a, b]
    ta = pt.Temporal(size, size)
    d_frame, d_counts, d_motion = pt.DeviceBuffer(frames[0].nbytes), pt.DeviceBuffer(size * size * 4), pt.DeviceBuffer(size * size * 16)
    try:
        ta.motion(scenes[1], scenes[0], basis, out=d_motion)
        pt.check(pt.lib.pt_device_synchronize())
        hit = float((d_motion.download(np.float32, (size, size, 4))[..., 3] >= 0).mean())
        res = {"hit_share": hit}
        res["static_ms"], res["static_ms_min"] = median_window(
            lambda k: ta.run(d_frame.ptr, SPP, basis, d_counts=d_counts.ptr), frames, d_frame, runs, warmup)
        res["motion_ms"], res["motion_ms_min"] = median_window(
            lambda k: ta.run(d_frame.ptr, SPP, basis, d_counts=d_counts.ptr, motion=d_motion), frames, d_frame, runs, warmup)
        res["scene_ms"], res["scene_ms_min"] = median_window(
            lambda k: ta.run(d_frame.ptr, SPP, basis, d_counts=d_counts.ptr, spheres=scenes[k]), frames, d_frame, runs, warmup)
        res["motion_kernel_ms"] = res["scene_ms"] - res["motion_ms"]
        # pt_temporal_motion alone (it has no timed twin): `runs` calls back to back between two device synchronisations, host
        # clock; each call stages, uploads and launches, so this is its throughput, upload and ring waits included
        batch = []
        for _ in range(5):
            pt.check(pt.lib.pt_device_synchronize())
            t0 = time.perf_counter()
            for i in range(runs):
                ta.motion(scenes[i % 2], scenes[1 - i % 2], basis, out=d_motion)
            pt.check(pt.lib.pt_device_synchronize())
            batch.append((time.perf_counter() - t0) * 1e3 / runs)
        res["motion_call_ms"] = float(np.median(batch))
        res["workspace_bytes"] = ta.memory()["workspace"]
    finally:
        for d in (d_frame, d_counts, d_motion):
            d.free()
        ta.destroy()
    return res


def static_vs_parent(pt, other, size, windows, runs, warmup, parent_first=False):
    frames, _, basis = two_frames(pt, size)
    out = {"new": [], "parent": []}
    sessions = {}
    # (the order decides where each session's history lies in device memory, which a memory-bound kernel can feel)
    for name, m in (("parent", other), ("new", pt)) if parent_first else (("new", pt), ("parent", other)):
        m.set_device(0)
        sessions[name] = (m, m.Temporal(size, size), m.DeviceBuffer(frames[0].nbytes), m.DeviceBuffer(size * size * 4))
    try:
        for w in range(windows):
            for name in ("new", "parent") if w % 2 == 0 else ("parent", "new"):
                m, ta, d_frame, d_counts = sessions[name]
                med, _ = median_window(lambda k: ta.run(d_frame.ptr, SPP, basis, d_counts=d_counts.ptr), frames, d_frame, runs,
                                       warmup if w == 0 else 2)
                out[name].append(med)
    finally:
        for m, ta, d_frame, d_counts in sessions.values():
            d_frame.free()
            d_counts.free()
            ta.destroy()
    new, parent = np.array(out["new"]), np.array(out["parent"])
    return {"windows_new_ms": out["new"], "windows_parent_ms": out["parent"], "new_ms": float(np.median(new)),
            "parent_ms": float(np.median(parent)), "difference_ms": float(np.median(new) - np.median(parent)),
            "parent_spread_ms": float(parent.max() - parent.min()), "new_spread_ms": float(new.max() - new.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[512, 1024])
    ap.add_argument("--spheres", nargs="+", type=int, default=[9, 1000])
    ap.add_argument("--runs", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent's session before this build's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    pt = ge.load_package()
    pt.set_device(0)
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
           "frame": f"Cornell box, {SPP} spp, sphere 7 moved between two frames"}
    if a.parent_lib:
        other = load_other(a.parent_lib)
        res.update(parent_fingerprint=other.build_fingerprint(), windows=a.windows, static={})
        for size in a.sizes:
            e = static_vs_parent(pt, other, size, a.windows, a.runs, a.warmup, a.parent_first)
            res["static"][str(size)] = e
            print(f"static {size}x{size}: new {e['new_ms']:.4f} ms, parent {e['parent_ms']:.4f} ms, difference {e['difference_ms']:+.4f} ms, "
                  f"parent's own spread {e['parent_spread_ms']:.4f} ms", flush=True)
        res["parent_first"] = a.parent_first
        name = "static_vs_parent_first.json" if a.parent_first else "static_vs_parent.json"
    else:
        res["cases"] = {}
        for size in a.sizes:
            for n in a.spheres:
                e = time_motion(pt, size, n, a.runs, a.warmup)
                res["cases"][f"{size}:{n}"] = e
                print(f"{size}x{size}, {n} spheres: static {e['static_ms']:.4f} ms, MOTION accumulate {e['motion_ms']:.4f} ms, scene call "
                      f"{e['scene_ms']:.4f} ms -> motion kernel {e['motion_kernel_ms']:.4f} ms; pt_temporal_motion alone {e['motion_call_ms']:.4f} ms per call "
                      f"(rays that hit: {e['hit_share']:.3f})", flush=True)
        name = "temporal_motion_time.json"
    if a.out:
        with open(os.path.join(a.out, name), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
