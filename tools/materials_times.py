#!/usr/bin/env python3
"""Kernel time of the materials kernel (csrc/pt_materials.hip) beside the ordinary renderer's automatic kernel: the Cornell box at
1024 x 1024 x 64 spp, 5 bounces, in one process, the arms alternating.

  plain        no material table: the kernel the automatic policy picks (the parent commit's diffuse kernel on this frame)
  all_diffuse  a table of nine DIFFUSE entries: the materials kernel on the same paths (the frames are bit-identical; checked)
  smallpt      SMALLPT_MATERIALS: sphere 6 a mirror, sphere 7 glass

Times are pt_renderer_render's own (a hipEvent pair around the launch), per arm the median, smallest and largest of the rounds
after the warm-up.  Writes profiles/materials/materials_times.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials", "materials_times.json"))
    args = ap.parse_args()
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("materials_times: no HIP device (a time is measured on the GPU or not at all)")
    pt.set_device(0)
    size, spp = args.size, args.spp
    spheres = pt.scene_cornell()
    basis = pt.camera_basis(width=size, height=size)
    d_scene, n = pt.upload_scene(spheres)
    tables = {"plain": None, "all_diffuse": [(pt.MATERIAL_DIFFUSE, 0.0)] * n, "smallpt": pt.SMALLPT_MATERIALS}
    result = {"device": pt.device_info(), "fingerprint": pt.build_fingerprint(), "size": size, "spp": spp, "max_bounces": 5,
              "rounds": args.rounds, "warmup": args.warmup, "arms": {}}
    for rng_name, rng in (("xorwow", pt.RNG_XORWOW), ("philox", pt.RNG_PHILOX)):
        arms = {}
        for name, table in tables.items():
            r = pt.Renderer(size, size, spp, rng_mode=rng, persist_rng=False)  # every frame from the seeded stream: equal work per round
            if table is not None:
                r.set_materials(table)
            arms[name] = (r, pt.DeviceBuffer(r.tile_floats * 4), [])
        for k in range(args.warmup + args.rounds):
            for name, (r, d_out, ms) in arms.items():
                t = r.render(d_out.ptr, d_scene.ptr, n, basis)
                if k >= args.warmup:
                    ms.append(t)
        frames = {name: d_out.download(np.float32, (size, size, 14)) for name, (r, d_out, ms) in arms.items()}
        same = bool(np.array_equal(frames["plain"].view(np.uint32), frames["all_diffuse"].view(np.uint32)))
        for name, (r, d_out, ms) in arms.items():
            info = r.kernel_info(n)
            result["arms"][f"{rng_name}/{name}"] = {
                "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "variant": info["variant"],
                "num_vgprs": info["num_vgprs"], "scratch_bytes": info["scratch_bytes"], "lds_bytes": info["lds_bytes"],
                "mean_colour": [float(x) for x in frames[name][..., :3].mean(axis=(0, 1))]}
            d_out.free()
            r.destroy()
        result[f"{rng_name}_all_diffuse_equals_plain"] = same
        base = result["arms"][f"{rng_name}/plain"]["median_ms"]
        for name in ("all_diffuse", "smallpt"):
            result["arms"][f"{rng_name}/{name}"]["over_plain"] = result["arms"][f"{rng_name}/{name}"]["median_ms"] / base
    d_scene.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
