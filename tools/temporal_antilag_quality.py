#!/usr/bin/env python3
"""Prints the quality tables of the temporal accumulator's responsive history (DENOISER.md, "Responsive history";
profiles/temporal_antilag/README.md): the float32 model on CPU oracle frames, no GPU.  The sequences and the measure are those of
tests/test_temporal_antilag_host.py (lamp_sequence, static_sequence, quality).

  python3 tools/temporal_antilag_quality.py [--ref-spp 256] [--sweep] [--fast-cap 8] [--hard-lamp]

Sequences: the lamp at 64 x 64 (8 frames, camera at rest) and at 128 x 128 (12 frames along temporal_model.fly_pose(k)), and the
static fly-through (128 x 128, 12 poses, its last frame against 2048 spp).  First the lamp scene's own figures: how much
consecutive references differ against the references' noise, and the share of the static-surface mask.  Then, per sequence, the
clamped-colour RMS error of the last frame, whole frame / static-surface mask, for (a) no accumulation, (b) plain accumulation at
cap 256, (c) plain accumulation at cap = fast_cap, (d) anti-lag at cap 256.  --sweep: (d) for clamp_sigma in {1, 1.5, 2, 3},
clamp_radius in {1, 2, 3}, fast_cap in {2n, 4n, 8n}, and the pair the rule of DENOISER.md picks."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import filter_model as fm  # noqa: E402
import temporal_antilag_model as am  # noqa: E402
import temporal_model as tm  # noqa: E402
import test_temporal_antilag_host as host  # noqa: E402

SIGMAS, RADII = (1.0, 1.5, 2.0, 3.0), (1, 2, 3)


def scene_figures(name, seq, size, noise_frame):
    """Consecutive references' clamped-colour RMS difference (its smallest value over the sequence) against the RMS between two
    references of one frame from different seeds, and the mask's share in the last frame."""
    steps = [fm.clamped_rms(seq[k][1], seq[k - 1][1]) for k in range(1, len(seq))]
    noise = fm.clamped_rms(seq[noise_frame][1], seq[noise_frame][5])
    mask = am.static_mask(size, size, seq[-1][4], seq[-1][2], seq[-1][3])
    if all(np.array_equal(seq[0][2], item[2]) and np.array_equal(seq[0][3], item[3]) for item in seq):  # camera at rest
        masks = [am.static_mask(size, size, item[4], item[2], item[3]) for item in seq]
        on = [fm.clamped_rms(seq[k][1][masks[k] & masks[k - 1]], seq[k - 1][1][masks[k] & masks[k - 1]]) for k in range(1, len(seq))]
        on_noise = fm.clamped_rms(seq[noise_frame][1][masks[noise_frame]], seq[noise_frame][5][masks[noise_frame]])
        print(f"{name}: on the static surfaces alone (both frames' masks) {min(on):.4f} .. {max(on):.4f} against {on_noise:.4f}: "
              f"{min(on) / on_noise:.1f} x", flush=True)
    print(f"{name}: consecutive references differ by {min(steps):.4f} .. {max(steps):.4f} RMS, two references of frame {noise_frame} by "
          f"{noise:.4f}: {min(steps) / noise:.1f} x; static-surface mask {mask.mean():.3f} of the frame", flush=True)


def cell(e):
    return f"{e[0]:.4f} / {e[1]:.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--fast-cap", type=float, default=host.FAST_CAP)
    ap.add_argument("--hard-lamp", action="store_true", help="the lamp of the recorded limit (temporal_antilag_model.HARD_LAMP)")
    a = ap.parse_args()
    if a.hard_lamp:
        am.LAMP.update(am.HARD_LAMP)
    oracle = ge.load_oracle()
    oracle.build()
    n = host.SPP
    lamp64 = host.lamp_sequence(oracle, 64, 8, n, a.ref_spp, host.STILL, noise_frame=4)
    lamp128 = host.lamp_sequence(oracle, 128, 12, n, a.ref_spp, tm.fly_pose, noise_frame=6)
    static = host.static_sequence(oracle)
    print(f"lamp: {am.LAMP}")
    scene_figures("lamp 64², 8 frames, camera at rest", lamp64, 64, 4)
    scene_figures("lamp 128², 12 frames along fly_pose(k)", lamp128, 128, 6)
    sequences = (("lamp 64², 8 frames, camera at rest", lamp64, 64), ("lamp 128², 12 frames along fly_pose(k)", lamp128, 128),
                 ("static 128², 12 poses along fly_pose(k)", static, 128))
    print(f"\nfast_cap {a.fast_cap:g}, clamp_sigma {am.DEFAULT_SIGMA:g}, clamp_radius {am.DEFAULT_RADIUS}: whole frame / static surfaces\n")
    print("| sequence | (a) none | (b) plain, cap 256 | (c) plain, cap = fast_cap | (d) anti-lag, cap 256 | (d) / (b) |")
    print("|---|---:|---:|---:|---:|---:|")
    plain = {}
    for name, seq, size in sequences:
        q = plain[name] = host.quality(seq, n, size, fast_cap=a.fast_cap)
        print(f"| {name} | {cell(q['a'])} | {cell(q['b'])} | {cell(q['c'])} | {cell(q['d'])} | {q['d'][0] / q['b'][0]:.4f} |", flush=True)
    if not a.sweep:
        return
    print("\nsweep: (d), whole frame / static surfaces; static cost = (d) / (b) over the whole last frame of the static fly-through\n")
    print("| fast_cap | clamp_sigma | clamp_radius | lamp 64² | lamp 128² | static 128² | static cost |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    rows = []
    for fast_cap in (2.0 * n, 4.0 * n, 8.0 * n):
        for k in SIGMAS:
            for R in RADII:
                d = [host.quality(seq, n, size, fast_cap=fast_cap, clamp_sigma=k, clamp_radius=R, plain=plain[name])["d"]
                     for name, seq, size in sequences]
                cost = d[2][0] / plain[sequences[2][0]]["b"][0]
                rows.append((fast_cap, k, R, d, cost))
                print(f"| {fast_cap:g} | {k:g} | {R} | {cell(d[0])} | {cell(d[1])} | {cell(d[2])} | {cost:.4f} |", flush=True)
    print("\nthe rule: per (clamp_sigma, clamp_radius) the static cost is the largest over the three fast_caps and the lamp error the mean"
          " of the lamp masks' (d) over both lamp sequences and the three fast_caps; among the pairs whose cost is within 5 % of the"
          " smallest, the smallest lamp error\n")
    pairs = {}
    for fast_cap, k, R, d, cost in rows:
        p = pairs.setdefault((k, R), dict(cost=0.0, lamp=[]))
        p["cost"] = max(p["cost"], cost)
        p["lamp"] += [d[0][1], d[1][1]]
    best_cost = min(p["cost"] for p in pairs.values())
    print("| clamp_sigma | clamp_radius | static cost | lamp mask error | eligible |")
    print("|---:|---:|---:|---:|---|")
    chosen = None
    for (k, R), p in sorted(pairs.items()):
        lamp = sum(p["lamp"]) / len(p["lamp"])
        ok = p["cost"] <= 1.05 * best_cost
        if ok and (chosen is None or lamp < chosen[2]):
            chosen = (k, R, lamp)
        print(f"| {k:g} | {R} | {p['cost']:.4f} | {lamp:.4f} | {'yes' if ok else 'no'} |")
    print(f"\nchosen: clamp_sigma {chosen[0]:g}, clamp_radius {chosen[1]}")


if __name__ == "__main__":
    main()
