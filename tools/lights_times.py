#!/usr/bin/env python3
"""Direct light sampling (csrc/pt_materials.hip, PT_VARIANT_MATERIALS_LIGHTS) measured on the device: what it costs and what it buys.

Time: 1024 x 1024 x 64 spp, 5 bounces, the recipe of tools/materials_times.py -- the arms alternate round by round in one process,
per arm the median, smallest and largest kernel time of pt_renderer_render.  Arms, per scene (the reference's box; the small-lamp
box: sphere 8 replaced by radius 1.5 at (50, 65.1, 81.6), emission 400) and generator:
  v101      an all-diffuse table, the option off (PT_VARIANT_MATERIALS)
  v102      the same table, the option on
  v101_sm   SMALLPT_MATERIALS, off;  v102_sm  on

Quality (--quality-size, default 512): clamped-colour RMS error (pt_compare, on the device) of a frame of --quality-spp samples
with the option on and off at EQUAL SPP, and of the frame without the option at EQUAL TIME (spp scaled by the measured time ratio
at that size), against a reference of --reference-frames x 1024 spp WITHOUT the option (frames of different seeds, averaged in
float64); for the small-lamp box, whose reference without the option is itself noisy, also against the same number of samples
WITH the option (the same expectation).  Writes profiles/lights/lights_times.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def small_lamp_box(box):
    s = box.copy()
    s[8] = (1.5, (50.0, 65.1, 81.6), (400.0, 400.0, 400.0), (0.0, 0.0, 0.0))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality-size", type=int, default=512)
    ap.add_argument("--quality-spp", type=int, default=16)
    ap.add_argument("--reference-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights", "lights_times.json"))
    args = ap.parse_args()
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("lights_times: no HIP device (a time is measured on the GPU or not at all)")
    pt.set_device(0)
    size, spp = args.size, args.spp
    scenes = {"reference_box": pt.scene_cornell(), "small_lamp_box": small_lamp_box(pt.scene_cornell())}
    result = {"device": pt.device_info(), "fingerprint": pt.build_fingerprint(), "size": size, "spp": spp, "max_bounces": 5,
              "rounds": args.rounds, "warmup": args.warmup, "arms": {}, "quality": {}}
    diffuse = [(pt.MATERIAL_DIFFUSE, 0.0)] * 9
    arm_defs = {"v101": (diffuse, False), "v102": (diffuse, True), "v101_sm": (pt.SMALLPT_MATERIALS, False), "v102_sm": (pt.SMALLPT_MATERIALS, True)}

    def renderer(sz, n_spp, table, lights, rng=pt.RNG_XORWOW, seed=0):
        r = pt.Renderer(sz, sz, n_spp, rng_mode=rng, persist_rng=False, seed=seed)  # every frame from the seeded stream: equal work per round
        if table is not None:
            r.set_materials(table)
        if lights:
            r.set_light_sampling(True)
        return r

    # ---- time ----
    basis = pt.camera_basis(width=size, height=size)
    for scene_name, spheres in scenes.items():
        d_scene, n = pt.upload_scene(spheres)
        for rng_name, rng in (("xorwow", pt.RNG_XORWOW), ("philox", pt.RNG_PHILOX)):
            arms = {}
            for name, (table, lights) in arm_defs.items():
                r = renderer(size, spp, table, lights, rng)
                arms[name] = (r, pt.DeviceBuffer(r.tile_floats * 4), [])
            for k in range(args.warmup + args.rounds):
                for name, (r, d_out, ms) in arms.items():
                    t = r.render(d_out.ptr, d_scene.ptr, n, basis)
                    if k >= args.warmup:
                        ms.append(t)
            for name, (r, d_out, ms) in arms.items():
                info = r.kernel_info(n)
                frame = d_out.download(np.float32, (size, size, 14))
                result["arms"][f"{scene_name}/{rng_name}/{name}"] = {
                    "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "variant": info["variant"],
                    "num_vgprs": info["num_vgprs"], "scratch_bytes": info["scratch_bytes"], "lds_bytes": info["lds_bytes"],
                    "mean_colour": [float(x) for x in frame[..., :3].astype(np.float64).mean(axis=(0, 1))],
                    "mean_colour_variance": float(frame[..., 10].astype(np.float64).mean())}
                d_out.free()
                r.destroy()
            for on, off in (("v102", "v101"), ("v102_sm", "v101_sm")):
                a = result["arms"]
                a[f"{scene_name}/{rng_name}/{on}"]["over_off"] = a[f"{scene_name}/{rng_name}/{on}"]["median_ms"] / a[f"{scene_name}/{rng_name}/{off}"]["median_ms"]
        d_scene.free()

    # ---- quality ----
    qs, qspp = args.quality_size, args.quality_spp
    basis = pt.camera_basis(width=qs, height=qs)
    cmp_ = pt.Compare(qs, qs)
    for scene_name, spheres in scenes.items():
        d_scene, n = pt.upload_scene(spheres)

        def frame(n_spp, lights, seed, rounds=1):
            r = renderer(qs, n_spp, None, lights, seed=seed)
            d_out = pt.DeviceBuffer(r.tile_floats * 4)
            ms = [r.render(d_out.ptr, d_scene.ptr, n, basis) for _ in range(rounds)]
            img = d_out.download(np.float32, (qs, qs, 14))
            d_out.free()
            r.destroy()
            return img, float(np.median(ms))

        refs = {}
        for lights in (False, True):
            acc = np.zeros((qs, qs, 3), dtype=np.float64)
            for f in range(args.reference_frames):
                acc += frame(1024, lights, 1000 + f)[0][..., :3]
            refs[lights] = (acc / args.reference_frames).astype(np.float32)
        on, t_on = frame(qspp, True, 1, rounds=7)
        off, t_off = frame(qspp, False, 1, rounds=7)
        spp_eq = max(1, int(round(qspp * t_on / t_off)))
        off_eq, t_off_eq = frame(spp_eq, False, 1, rounds=7)
        q = {"size": qs, "spp": qspp, "reference_spp": 1024 * args.reference_frames, "ms_on": t_on, "ms_off": t_off, "equal_time_spp_off": spp_eq,
             "ms_off_equal_time": t_off_eq,
             "rms_between_the_two_references": pt.compare_frames(refs[True], refs[False], compare=cmp_)["rms"]}
        for ref_name, ref in (("against_reference_without", refs[False]), ("against_reference_with", refs[True])):
            q[ref_name] = {"on": pt.compare_frames(on[..., :3], ref, compare=cmp_)["rms"],
                           "off_equal_spp": pt.compare_frames(off[..., :3], ref, compare=cmp_)["rms"],
                           "off_equal_time": pt.compare_frames(off_eq[..., :3], ref, compare=cmp_)["rms"]}
        result["quality"][scene_name] = q
        d_scene.free()
    cmp_.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
