#!/usr/bin/env python3
"""Sky and sun (csrc/pt_materials.hip, PT_VARIANT_MATERIALS_SKY / PT_VARIANT_MATERIALS_LIGHTS_SKY) measured on the device: what a sky
costs and what sampling the sun buys.  The recipe of tools/lights_times.py.

Time: 1024 x 1024 x 64 spp, 5 bounces -- the arms alternate round by round in one process, per arm the median, smallest and largest
kernel time of pt_renderer_render.  Scenes: the courtyard (a floor of radius 1e4 and the reference's two balls, all DIFFUSE) and
scene_random(40, with_walls=False); both generators.  Arms:
  v101        an all-diffuse table, no sky (PT_VARIANT_MATERIALS)          v103        the same under CLEAR_SKY
  v102        light sampling on, no sky (PT_VARIANT_MATERIALS_LIGHTS)      v104        the same under CLEAR_SKY: the sun is sampled
  v104_sunless  light sampling on under CLEAR_SKY's gradient without its sun

Quality (--quality-size, default 512): clamped-colour RMS error (pt_compare, on the device) of a courtyard frame of --quality-spp
samples under CLEAR_SKY with sun sampling on and off at EQUAL SPP, and off at EQUAL TIME (spp scaled by the measured time ratio at
that size), against a reference of --reference-frames x 1024 spp WITH sampling (frames of different seeds, averaged in float64), and
against the same number of samples WITHOUT it (the same expectation, a noisier reference: the RMS between the two is given).

--ab PACKAGE LABEL: instead of all that, ONE JSON line for comparing two builds of the library (this commit's and its parent's, run
in turn as separate processes): the reference's box at 1024 x 1024 x 64 spp, the four builds without a sky -- 101 and 102, both
generators, all-diffuse table -- alternating round by round, with a checksum of each last frame.  PACKAGE is a directory holding
that build's __init__.py, denoise_weights.py and libptcore.so.

Writes profiles/sky/sky_times.json (or --out)."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(pkg):
    if pkg is None:
        import __graft_entry__ as ge

        return ge.load_package()
    pkg = os.path.abspath(pkg)
    spec = importlib.util.spec_from_file_location("ptpkg_ab", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    pt = importlib.util.module_from_spec(spec)
    sys.modules["ptpkg_ab"] = pt
    spec.loader.exec_module(pt)
    return pt


def courtyard(pt):
    box = pt.scene_cornell()
    s = np.zeros(3, dtype=box.dtype)
    s[0] = (1e4, (50.0, -1e4, 81.6), (0.0, 0.0, 0.0), (0.75, 0.75, 0.75))
    s[1], s[2] = box[6], box[7]
    return s


def timed(pt, arms, d_scene, n, basis, warmup, rounds, size):
    """arms: {name: renderer}.  Alternating rounds; {name: record}."""
    bufs = {name: (r, pt.DeviceBuffer(r.tile_floats * 4), []) for name, r in arms.items()}
    for k in range(warmup + rounds):
        for name, (r, d_out, ms) in bufs.items():
            t = r.render(d_out.ptr, d_scene.ptr, n, basis)
            if k >= warmup:
                ms.append(t)
    out = {}
    for name, (r, d_out, ms) in bufs.items():
        info = r.kernel_info(n)
        frame = d_out.download(np.float32, (size, size, 14))
        out[name] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "variant": info["variant"],
                     "num_vgprs": info["num_vgprs"], "scratch_bytes": info["scratch_bytes"], "lds_bytes": info["lds_bytes"],
                     "frame_crc": int(np.bitwise_xor.reduce(frame.view(np.uint32).reshape(-1))),
                     "mean_colour": [float(x) for x in frame[..., :3].astype(np.float64).mean(axis=(0, 1))],
                     "mean_colour_variance": float(frame[..., 10].astype(np.float64).mean())}
        d_out.free()
        r.destroy()
    return out


def ab(args):
    pt = load(args.ab[0])
    if pt.device_count() < 1:
        raise SystemExit("sky_times: no HIP device (a time is measured on the GPU or not at all)")
    pt.set_device(0)
    size, spp = 1024, 64
    d_scene, n = pt.upload_scene(pt.scene_cornell())
    basis = pt.camera_basis(width=size, height=size)
    arms = {}
    for rng_name, rng in (("xorwow", pt.RNG_XORWOW), ("philox", pt.RNG_PHILOX)):
        for name, lights in (("v101", False), ("v102", True)):
            r = pt.Renderer(size, size, spp, rng_mode=rng, persist_rng=False)
            r.set_materials([(0, 0.0)] * 9)
            if lights:
                r.set_light_sampling(True)
            arms[f"{rng_name}/{name}"] = r
    rec = timed(pt, arms, d_scene, n, basis, args.warmup, args.rounds, size)
    d_scene.free()
    out = {"label": args.ab[1], "fingerprint": pt.build_fingerprint()}
    out.update({k: {f: v[f] for f in ("median_ms", "min_ms", "max_ms", "variant", "frame_crc")} for k, v in rec.items()})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality-size", type=int, default=512)
    ap.add_argument("--quality-spp", type=int, default=16)
    ap.add_argument("--reference-frames", type=int, default=16)
    ap.add_argument("--ab", nargs=2, metavar=("PACKAGE", "LABEL"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky", "sky_times.json"))
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    pt = load(None)
    if pt.device_count() < 1:
        raise SystemExit("sky_times: no HIP device (a time is measured on the GPU or not at all)")
    pt.set_device(0)
    size, spp = args.size, args.spp
    clear = pt.CLEAR_SKY
    sunless = pt.Sky(clear.zenith, clear.horizon, clear.ground)
    scenes = {"courtyard": courtyard(pt), "random40_open": pt.scene_random(40, 1, with_walls=False)}
    result = {"device": pt.device_info(), "fingerprint": pt.build_fingerprint(), "size": size, "spp": spp, "max_bounces": 5, "rounds": args.rounds,
              "warmup": args.warmup, "clear_sky": clear.as_dict(), "arms": {}, "quality": {}}
    arm_defs = {"v101": (False, None), "v103": (False, clear), "v102": (True, None), "v104": (True, clear), "v104_sunless": (True, sunless)}

    def renderer(sz, n_spp, n_spheres, lights, sky, rng=pt.RNG_XORWOW, seed=0, table=True):
        r = pt.Renderer(sz, sz, n_spp, rng_mode=rng, persist_rng=False, seed=seed)  # every frame from the seeded stream: equal work per round
        if table:
            r.set_materials([(pt.MATERIAL_DIFFUSE, 0.0)] * n_spheres)
        if lights:
            r.set_light_sampling(True)
        if sky is not None:
            r.set_sky(sky)
        return r

    # ---- time ----
    basis = pt.camera_basis(width=size, height=size)
    for scene_name, spheres in scenes.items():
        d_scene, n = pt.upload_scene(spheres)
        for rng_name, rng in (("xorwow", pt.RNG_XORWOW), ("philox", pt.RNG_PHILOX)):
            rec = timed(pt, {name: renderer(size, spp, n, lights, sky, rng) for name, (lights, sky) in arm_defs.items()}, d_scene, n, basis,
                        args.warmup, args.rounds, size)
            for on, off in (("v103", "v101"), ("v104", "v102"), ("v104", "v104_sunless")):
                rec[on]["over_" + off] = rec[on]["median_ms"] / rec[off]["median_ms"]
            for name, r in rec.items():
                result["arms"][f"{scene_name}/{rng_name}/{name}"] = r
        d_scene.free()

    # ---- quality ----
    qs, qspp = args.quality_size, args.quality_spp
    basis = pt.camera_basis(width=qs, height=qs)
    cmp_ = pt.Compare(qs, qs)
    d_scene, n = pt.upload_scene(scenes["courtyard"])

    def frame(n_spp, lights, seed, rounds=1):
        r = renderer(qs, n_spp, n, lights, clear, seed=seed, table=False)
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
         "ms_off_equal_time": t_off_eq, "rms_between_the_two_references": pt.compare_frames(refs[True], refs[False], compare=cmp_)["rms"],
         "mean_colour_variance": {"on": float(on[..., 10].astype(np.float64).mean()), "off": float(off[..., 10].astype(np.float64).mean())}}
    for ref_name, ref in (("against_reference_with", refs[True]), ("against_reference_without", refs[False])):
        q[ref_name] = {"on": pt.compare_frames(on[..., :3], ref, compare=cmp_)["rms"],
                       "off_equal_spp": pt.compare_frames(off[..., :3], ref, compare=cmp_)["rms"],
                       "off_equal_time": pt.compare_frames(off_eq[..., :3], ref, compare=cmp_)["rms"]}
    result["quality"]["courtyard_clear_sky"] = q
    d_scene.free()
    cmp_.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
