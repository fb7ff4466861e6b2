#!/usr/bin/env python3
"""Prints the quality table of temporal accumulation with moving spheres (DENOISER.md, "Moving spheres";
profiles/temporal_motion/README.md): the float32 model on CPU oracle frames, no GPU.  The sequences and the measure are those of
tests/test_temporal_motion_host.py (moving_sequence, quality), which asserts the ordering on the first row only.

  python3 tools/temporal_motion_quality.py [--ref-spp 256]

Rows: 64 x 64, 6 frames, camera at rest, and 128 x 128, 12 frames along temporal_model.fly_pose(k), each with history_cap 256
and 8.  Columns: clamped-colour RMS error of the last frame, whole frame / the moving sphere's pixels, for (a) no accumulation,
(b) accumulation blind to the motion, (c) accumulation with motion.  About ten seconds on 16 cores."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge  # noqa: E402
import temporal_model as tm  # noqa: E402
import test_temporal_motion_host as host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=256)
    a = ap.parse_args()
    oracle = ge.load_oracle()
    oracle.build()
    print("| sequence | cap | (a) frame / sphere | (b) frame / sphere | (c) frame / sphere |")
    print("|---|---:|---:|---:|---:|")
    for name, size, frames, pose in (("64², 6 frames, camera at rest", 64, 6, lambda k: ((50.0, 52.0, 295.6), -90.0)),
                                     ("128², 12 frames along fly_pose(k)", 128, 12, tm.fly_pose)):
        seq = host.moving_sequence(oracle, size, frames, 4, a.ref_spp, pose)
        for cap in (256.0, 8.0):
            q = host.quality(seq, 4, size, history_cap=cap)
            cells = " | ".join(f"{q[k][0]:.4f} / {q[k][1]:.4f}" for k in ("none", "blind", "motion"))
            print(f"| {name} | {cap:g} | {cells} |", flush=True)


if __name__ == "__main__":
    main()
