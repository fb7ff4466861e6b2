#!/usr/bin/env python3
"""Times progressive passes (pt_progressive_*, pixel_kernel's resume builds) against the single launches they replace:
  * cfg5 shape (512^2, reference scene, 8 bounces): a pass of 4 spp against a Render() of 4 spp, alternating windows of
    --window launches each (wall time per launch over the window, device synchronised at both ends); min / median / max;
  * headline (1024^2, 5 bounces): 4 passes of 256 against one 1024-spp Render() (device-event ms, summed over the passes);
  * config 4 (1024^2, 1000 random spheres, closed): 4 x 64 against 256.
Writes progressive_time.json (kernel resources of the builds: kernel_resources.txt beside it, from -Rpass-analysis).

  python3 tools/progressive_time.py [--window 1000] [--windows 5] [--reps 3] [--out profiles/progressive]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "runs": len(xs)}


def cfg5(pt, args):
    w = h = 512
    scene = pt.scene_cornell()
    basis = pt.camera_basis(width=w, height=h)
    d_scene, ns = pt.upload_scene(scene)
    d_out = pt.DeviceBuffer(w * h * 56)
    r = pt.Renderer(w, h, 4, max_bounces=8)
    s = pt.Progressive(r)
    t_render, t_pass = [], []
    for _ in range(args.windows):
        pt.lib.pt_device_synchronize()
        t0 = time.perf_counter()
        for _ in range(args.window):
            r.enqueue(d_out.ptr, d_scene.ptr, ns, basis)
        pt.lib.pt_device_synchronize()
        t_render.append((time.perf_counter() - t0) * 1e3 / args.window)
        s.reset()
        pt.lib.pt_device_synchronize()
        t0 = time.perf_counter()
        for _ in range(args.window):
            s.enqueue(4, d_out.ptr, d_scene.ptr, ns, basis)
        pt.lib.pt_device_synchronize()
        t_pass.append((time.perf_counter() - t0) * 1e3 / args.window)
    res = {"shape": "512^2 x 4 spp, reference scene, 8 bounces", "render_variant": r.kernel_info(ns)["variant"],
           "pass_variant": s.variant(ns), "render_ms": stats(t_render), "pass_ms": stats(t_pass)}
    res["ratio_median"] = res["pass_ms"]["median"] / res["render_ms"]["median"]
    s.destroy()
    r.destroy()
    d_out.free()
    return res


def split(pt, args, name, scene, total, passes):
    w = h = 1024
    basis = pt.camera_basis(width=w, height=h)
    d_scene, ns = pt.upload_scene(scene)
    d_a, d_b = pt.DeviceBuffer(w * h * 56), pt.DeviceBuffer(w * h * 56)
    r1 = pt.Renderer(w, h, total)
    r2 = pt.Renderer(w, h, passes[0])
    s = pt.Progressive(r2)
    # warm-up, and the check: the renderer's FIRST frame (its XORWOW state persists, later frames differ) against the session
    r1.render(d_a.ptr, d_scene.ptr, ns, basis)
    for p in passes:
        s.render(p, d_b.ptr, d_scene.ptr, ns, basis)
    same = np.array_equal(d_a.download(np.float32, (h, w, 14)).view(np.uint32), d_b.download(np.float32, (h, w, 14)).view(np.uint32))
    t_one, t_split = [], []
    for _ in range(args.reps):
        t_one.append(r1.render(d_a.ptr, d_scene.ptr, ns, basis))
        s.reset()
        t_split.append(sum(s.render(p, d_b.ptr, d_scene.ptr, ns, basis) for p in passes))
    res = {"shape": name, "one_render": f"{total} spp", "passes": passes, "render_variant": r1.kernel_info(ns)["variant"],
           "pass_variant": s.variant(ns), "render_ms": stats(t_one), "passes_ms": stats(t_split), "bit_identical": bool(same)}
    res["ratio_median"] = res["passes_ms"]["median"] / res["render_ms"]["median"]
    s.destroy()
    r1.destroy()
    r2.destroy()
    for d in (d_a, d_b, d_scene):
        d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive"))
    args = ap.parse_args()
    pt = ge.load_package()
    pt.set_device(0)
    out = {"device": pt.device_info(), "build": pt.build_fingerprint(), "cfg5": cfg5(pt, args),
           "headline": split(pt, args, "1024^2 reference scene, 5 bounces", pt.scene_cornell(), 1024, [256] * 4),
           "config4": split(pt, args, "1024^2, 1000 random spheres, closed", pt.scene_random(1000, 1, True), 256, [64] * 4)}
    print(json.dumps(out, indent=1, default=str))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "progressive_time.json"), "w") as f:
        json.dump(out, f, indent=1, default=str)


if __name__ == "__main__":
    main()
