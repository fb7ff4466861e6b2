#!/usr/bin/env python3
"""The quality table of the feature filter's spatial variance estimate (DENOISER.md, "Spatial variance estimate"), from the
float64 NumPy models of tests/ on CPU oracle frames.  No GPU.

  python3 tools/filter_spatial_quality.py [--out DIR]        -> quality.txt
      clamped-colour RMS error against a 4096-spp frame of seed 12345: the plain filter and the estimate for every pixel at
      R = 1, 2, 3, at 1 .. 16 spp, for the 128^2 default camera and a 96^2 view from (30, 40, 200), yaw -75, pitch -10; then
      behind the temporal model on fly_pose(k), the filter fed the model's counts, below = 16, R = 2: 96^2 at 1 spp (10 frames)
      and 128^2 at 4 spp (6 frames).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge  # noqa: E402
import filter_model as fm  # noqa: E402
import filter_spatial_model as fsm  # noqa: E402
import temporal_model as tm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    oracle = ge.load_oracle()
    lines = ["clamped-colour RMS error against 4096 spp (seed 12345); float64 models; below = all",
             f"{'frame':34s} {'spp':>3s} {'plain':>7s} {'R=1':>7s} {'R=2':>7s} {'R=3':>7s} {'R=2 / plain':>11s}"]
    views = (("128^2 default camera", 128, None, {}), ("96^2 eye (30,40,200) yaw -75 pitch -10", 96, (30.0, 40.0, 200.0), dict(yaw=-75.0, pitch=-10.0)))
    for name, size, eye, pose in views:
        args = dict(basis=oracle.camera_basis(eye, w=size, h=size, **pose) if eye else oracle.camera_basis(w=size, h=size))
        if eye:
            args["eye"] = eye
        ref = oracle.render(size, size, 4096, seed=12345, **args)[..., :3]
        for spp in (1, 2, 4, 8, 16):
            frame = oracle.render(size, size, spp, **args)
            plain = fm.clamped_rms(fm.filter_model(frame, samples=spp), ref)
            e = [fm.clamped_rms(fsm.filter_model(frame, samples=spp, below=fsm.ALL, radius=R), ref) for R in (1, 2, 3)]
            lines.append(f"{name:34s} {spp:3d} {plain:7.4f} {e[0]:7.4f} {e[1]:7.4f} {e[2]:7.4f} {e[1] / plain:11.3f}")
            print(lines[-1], flush=True)
    lines += ["", "behind the temporal model on fly_pose(k): the filter gets the model's counts; below = 16, R = 2",
              f"{'run':14s} {'frame':>5s} {'plain':>7s} {'spatial':>7s} {'ratio':>6s}"]
    for name, size, n, frames in (("96^2, 1 spp", 96, 1, 10), ("128^2, 4 spp", 128, 4, 6)):
        state = oracle.setup_random(size, size)
        model = tm.TemporalModel(size, size)
        for k in range(frames):
            eye, yaw = tm.fly_pose(k)
            basis = oracle.camera_basis(eye, yaw=yaw, w=size, h=size)
            frame = oracle.render(size, size, n, basis=basis, eye=eye, rng_state=state)
            ref = oracle.render(size, size, 4096, basis=basis, eye=eye, seed=12345)[..., :3]
            acc, counts = model.accumulate(frame, n, basis, eye)
            plain = fm.clamped_rms(fm.filter_model(acc, counts=counts), ref)
            spatial = fm.clamped_rms(fsm.filter_model(acc, counts=counts, below=16, radius=2), ref)
            lines.append(f"{name:14s} {k:5d} {plain:7.4f} {spatial:7.4f} {spatial / plain:6.3f}")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        open(os.path.join(a.out, "quality.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
