"""Adaptive sampling of progressive sessions: what a pass costs against its active fraction, and what the samples buy.

  python3 tools/adaptive_time.py [--out profiles/adaptive/adaptive_time.json] [--reps 3] [--quick]

1. Pass cost (headline scene, 1024^2, 5 bounces, XORWOW): after a uniform first pass of 64 samples, a 64-spp pass of a plain
   session against an adaptive pass whose active set is forced (lab library) to random 8x8 tiles covering about 25 % of the
   frame, and to none at all (what selection + an empty launch + finalize cost).  Alternated runs, device-event times.
2. Quality (headline scene, 512^2): mean relMSE of the colour against a uniform high-spp GPU reference, uniform sessions
   against adaptive ones for several tolerances, as a function of the samples spent (sum of the per-pixel counts).
3. Config 4 (1000 random spheres, closed and open box, 256^2): the same comparison, shorter.
The reference renders with another seed, so that its samples are independent of the ones it judges."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def session(pt, w, h, spheres, spp_hint, rng=0, seed=0):
    r = pt.Renderer(w, h, spp_hint, rng_mode=rng, seed=seed)
    s = pt.Progressive(r)
    d_scene, ns = pt.upload_scene(spheres)
    d_out = pt.DeviceBuffer(w * h * 56)
    return r, s, d_scene, ns, d_out


def pass_cost(lab, reps):
    w = h = 1024
    basis = lab.camera_basis(width=w, height=h)
    rows = {"plain": [], "quarter": [], "none": []}
    frac = None
    rng = np.random.default_rng(1)
    tiles = rng.uniform(size=(h // 8, w // 8)) < 0.25
    quarter = np.kron(tiles, np.ones((8, 8), bool))
    for _ in range(reps):
        for kind in ("plain", "quarter", "none"):
            r, s, d_scene, ns, d_out = session(lab, w, h, lab.scene_cornell(), 64)
            if kind != "plain":
                s.set_adaptive(0.0, min_samples=1 << 30)
            s.render(64, d_out.ptr, d_scene.ptr, ns, basis)
            if kind == "quarter":
                s.set_active(quarter)
                frac = s.active() / (w * h)
            elif kind == "none":
                s.set_active(np.zeros((h, w), bool))
            ms = s.render(64, d_out.ptr, d_scene.ptr, ns, basis)
            rows[kind].append(ms)
            s.destroy()
            r.destroy()
            d_out.free()
            d_scene.free()
    return {"scene": "headline 1024^2, 5 bounces, xorwow, second pass of 64 spp", "active_fraction_quarter": frac,
            "ms": rows, "ratio_quarter_vs_plain": min(rows["quarter"]) / min(rows["plain"]),
            "select_empty_finalize_ms": min(rows["none"])}


def counts_np(pt, s, d_counts, n):
    """The session's per-pixel counts through a device buffer (pt_progressive_counts), as NumPy."""
    pt.check(pt.lib.pt_progressive_counts(s.handle, d_counts.ptr, None))
    pt.check(pt.lib.pt_device_synchronize())
    return d_counts.download(np.uint32, (n,))


def colour(pt, d_out, w, h):
    return d_out.download(np.float32, (h, w, 14))[..., :3].astype(np.float64)


def relmse(img, ref):
    return float(np.mean((img - ref) ** 2 / (ref ** 2 + 1e-2)))


def quality(pt, spheres, w, h, ref_spp, uniform, tolerances, pass_spp, budget, label):
    basis = pt.camera_basis(width=w, height=h)
    rr, s, d_scene, ns, d_out = session(pt, w, h, spheres, 64, seed=0x5EED)
    d_counts = pt.DeviceBuffer(w * h * 4)
    t0 = time.time()
    done = 0
    while done < ref_spp:  # the reference: one uniform session, passes of 1024
        s.render(min(1024, ref_spp - done), d_out.ptr, d_scene.ptr, ns, basis)
        done += min(1024, ref_spp - done)
    ref = colour(pt, d_out, w, h)
    ref_s = time.time() - t0
    s.destroy()
    rr.destroy()
    r = pt.Renderer(w, h, 64)
    out = {"scene": label, "size": [w, h], "reference_spp": ref_spp, "reference_s": ref_s, "uniform": [], "adaptive": []}
    s = pt.Progressive(r)
    n = 0
    for target in uniform:
        s.render(target - n, d_out.ptr, d_scene.ptr, ns, basis)
        n = target
        out["uniform"].append({"spp": n, "mean_spp": n, "relmse": relmse(colour(pt, d_out, w, h), ref)})
    s.destroy()
    for tol in tolerances:
        s = pt.Progressive(r)
        s.set_adaptive(tol)
        curve = []

        def on_pass(sess, k, ms):
            c = counts_np(pt, sess, d_counts, w * h)
            curve.append({"max_spp": int(c.max()), "mean_spp": float(c.mean()), "relmse": relmse(colour(pt, d_out, w, h), ref),
                          "active_after": sess.active() / (w * h), "ms": ms})

        s.refine(budget, pass_spp, d_out.ptr, d_scene.ptr, ns, basis, on_pass=on_pass)
        out["adaptive"].append({"tolerance": tol, "floor": pt.ADAPTIVE_FLOOR, "min_samples": pt.ADAPTIVE_MIN_SAMPLES,
                                "radius": pt.ADAPTIVE_RADIUS, "curve": curve})
        s.destroy()
    r.destroy()
    for d in (d_out, d_scene, d_counts):
        d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "adaptive_time.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    pt, lab = ge.load_package(), ge.load_lab()
    pt.set_device(0)
    lab.set_device(0)
    res = {"fingerprint": pt.build_fingerprint(), "device": pt.device_info()}
    res["pass_cost"] = pass_cost(lab, a.reps)
    print(json.dumps(res["pass_cost"]), flush=True)
    tols = [0.02, 0.03, 0.05, 0.08] if not a.quick else [0.05]
    uniform = [64, 128, 256, 512, 1024, 2048]
    res["quality_headline"] = quality(pt, pt.scene_cornell(), 512, 512, 16384 if not a.quick else 4096, uniform, tols, 32, 4096,
                                      "headline scene (Cornell box), 5 bounces")
    print(json.dumps({k: v for k, v in res["quality_headline"].items() if k != "adaptive"}), flush=True)
    for walls in (True, False):
        key = "quality_config4_" + ("closed" if walls else "open")
        res[key] = quality(pt, pt.scene_random(1000, 1, walls), 256, 256, 2048, [64, 128, 256, 512], [0.05], 32, 1024,
                           f"config 4 ({'closed' if walls else 'open'}), 1000 spheres, 256^2")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
