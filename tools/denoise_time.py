#!/usr/bin/env python3
"""Times pt_denoiser_enqueue (the reference's DenoiseCNN step, csrc/pt_denoise.hip) with device events around each run on a
rendered Cornell frame with random weights: warm-up, then the median of --runs runs per size.  In the same process it times
torch's own fp32 forward of the restated network (tests/denoise_restatement.py; torch/MIOpen, a comparison point only) and
lists every layer's shape and FLOPs (2 M N K, counted from the shapes; K with the 14 real input channels).

  python3 tools/denoise_time.py [--sizes 512 1024] [--runs 200] [--no-torch] [--out DIR]
  python3 tools/denoise_time.py --frames 1 8 32 --sizes 128 256 512 [--out DIR]
      batches: per-frame time of pt_denoiser_enqueue_frames of n frames (one group, max_frames = n; n = 1 is
      pt_denoiser_enqueue), the median of device-event windows around whole batches after warm-up -> frames_time.json
  python3 tools/denoise_time.py --trace DIR/..._kernel_trace.csv --sizes 512 [--frames 32] --out DIR
      per-layer kernel times from a rocprofv3 --kernel-trace run of this tool (dispatches mapped to layers in launch order;
      with --frames n, of a run with that one --frames value: every batch is one sequence of the same launches)
  --precision half|float selects the denoiser's mode for every timing and for the --trace layer table (default float); the
      table then also lists the bytes each layer has to move and its GB/s, and the workspace sizes of the mode
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

FLOOR_TFS = 157.3  # fp32 MFMA peak (MI355X_MICROARCH.md): 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


PRECISIONS = {"float": "float32", "half": "half"}  # command line name -> Denoiser(precision=...)


def layer_table(lab, w, h, sd, frames=1, precision="float32", memory=None):
    """[(name, M, N, K, flops, bytes, splits, tile)] in launch order, from the lab library's conv table (the plan of a group
    of `frames` frames: M, FLOPs and bytes of the whole group).  bytes = what the layer must move once: its input, weights,
    outputs, residual and coarse map at the mode's element size, plus the fp32 split-K partials written and read back.
    memory (a dict) receives the denoiser's workspace sizes."""
    dn = lab.Denoiser(w, h, sd, max_frames=frames, precision=precision)
    try:
        layers = dn.layers()
        plan = dn.conv_plan(frames)
        mem = dn.memory()
        if memory is not None:
            memory.update({k: mem[k] for k in ("element", "workspace", "partials", "weights")})
        esz = mem["element"]
        size = lambda i: frames * int(np.prod(layers[i][1])) * esz
        rows = []
        for (name, inf), p in zip(dn.convs(), plan):
            ih, iw, cin = layers[inf["in"]][1]
            cin_real = 14 if inf["in"] == 0 else cin
            oh, ow = (ih - 1) // inf["stride"] + 1, (iw - 1) // inf["stride"] + 1
            M, N, K = frames * oh * ow, inf["N"], inf["ks"] ** 2 * cin_real
            assert M == p["M"]
            nbytes = size(inf["in"]) + inf["ks"] ** 2 * cin * N * esz + sum(size(inf[k]) for k in ("out0", "out1", "res", "up") if inf[k] >= 0)
            if inf["out0"] < 0:
                nbytes += M * 3 * 4 + M * 3 * esz  # the head: fp32 rgb out, albedo in
            if p["splits"] > 1:
                nbytes += 2 * p["splits"] * M * N * 4
            rows.append(dict(name=name, M=M, N=N, K=K, flops=2.0 * M * N * K, bytes=nbytes, splits=p["splits"], tile=f'{p["bm"]}x{p["bn"]}'))
        return rows
    finally:
        dn.destroy()


def time_hip(pt, w, h, sd, runs, warmup, precision="float32"):
    import torch

    frame = pt.render_frame(w, h, 4)[0]
    d_src = torch.from_numpy(frame).cuda()
    d_frame = d_src.clone()
    dn = pt.Denoiser(w, h, sd, precision=precision)
    s = torch.cuda.current_stream()
    times = []
    try:
        for i in range(warmup + runs):
            d_frame.copy_(d_src)  # in place is the reference's mode: every run starts from the rendered frame
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            dn.enqueue(d_frame.data_ptr(), None, s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
    finally:
        torch.cuda.synchronize()
        dn.destroy()
    return np.array(times)


def time_hip_frames(pt, w, h, sd, n, runs, warmup, precision="float32"):
    """Device-event ms of whole batches of n frames (n different poses) through ONE enqueue_frames call each (n = 1:
    pt_denoiser_enqueue); every run starts from the rendered frames."""
    import torch

    frames = []
    for k in range(n):
        eye = (50.0 + 0.7 * k, 52.0 - 0.3 * k, 295.6 - 1.1 * k)
        basis = pt.camera_basis(eye, yaw=-90.0 + 0.9 * k, pitch=-0.4 * k, width=w, height=h)
        frames.append(pt.render_frame(w, h, 4, basis=basis, eye=eye)[0])
    d_src = torch.from_numpy(np.stack(frames)).cuda()
    d_frames = d_src.clone()
    dn = pt.Denoiser(w, h, sd, max_frames=n, precision=precision)
    s = torch.cuda.current_stream()
    times = []
    try:
        for i in range(warmup + runs):
            d_frames.copy_(d_src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if n == 1:
                dn.enqueue(d_frames.data_ptr(), None, s.cuda_stream)
            else:
                dn.enqueue_frames(d_frames.data_ptr(), n, stream=s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
    finally:
        torch.cuda.synchronize()
        dn.destroy()
    return np.array(times)


def time_torch(w, h, sd, runs, warmup):
    import torch

    import denoise_restatement as R

    pt = ge.load_package()
    frame = pt.render_frame(w, h, 4)[0]
    x = R.to_nchw(R.preprocess(frame), torch.float32).cuda()
    sdt = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    times = []
    with torch.no_grad():
        for i in range(warmup + runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            R.forward(x, sdt)
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
    return np.array(times)


def from_trace(path, rows):
    """Median kernel time of each layer from a rocprofv3 kernel trace: per frame the two pre-processing kernels, then per
    layer its conv kernel (+ the split-K reduction).  path: a kernel_trace.csv or a rocpd database (*_results.db, the
    default output of newer rocprofv3), whose `kernels` view carries the same three columns."""
    if path.endswith(".db"):
        import sqlite3

        with sqlite3.connect(path) as db:
            recs = [dict(Kernel_Name=n, Start_Timestamp=b, End_Timestamp=e) for n, b, e in db.execute("select name, start, end from kernels")]
    else:
        with open(path) as f:
            recs = list(csv.DictReader(f))
    key_name = next(k for k in recs[0] if k.lower() in ("kernel_name", "kernelname"))
    key_s = next(k for k in recs[0] if k.lower() in ("start_timestamp", "begin_ns", "start"))
    key_e = next(k for k in recs[0] if k.lower() in ("end_timestamp", "end_ns", "end"))
    recs = [r for r in recs if "ptdn" in r[key_name]]
    recs.sort(key=lambda r: int(r[key_s]))
    per_frame = 2 + sum(1 + (r["splits"] > 1) for r in rows)
    frames = len(recs) // per_frame
    out = {"pre_max + pre_apply": []}
    for r in rows:
        out[r["name"]] = []
    for f in range(frames):
        seq = recs[f * per_frame:(f + 1) * per_frame]
        assert "pre_max" in seq[0][key_name], seq[0][key_name]
        dur = lambda q: (int(q[key_e]) - int(q[key_s])) * 1e-6  # ns -> ms
        out["pre_max + pre_apply"].append(dur(seq[0]) + dur(seq[1]))
        i = 2
        for r in rows:
            t = dur(seq[i])
            i += 1
            if r["splits"] > 1:
                assert "splitk" in seq[i][key_name]
                t += dur(seq[i])
                i += 1
            out[r["name"]].append(t)
    return frames, {k: float(np.median(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=None)
    ap.add_argument("--precision", choices=sorted(PRECISIONS), default="float")
    a = ap.parse_args()
    precision = PRECISIONS[a.precision]
    tag = "" if precision == "float32" else "_half"
    if not a.trace:
        import torch

        torch.cuda.set_device(0)  # torch's HIP context first (as bench.py does), then the library's
    pt, lab = ge.load_package(), ge.load_lab()
    from cuda_pathtrace_amd import denoise_weights as dw

    sd = dw.random_state_dict(seed=1)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.trace:
        path = a.trace if os.path.isfile(a.trace) else sorted(glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
                                                              + glob.glob(os.path.join(a.trace, "**", "*_results.db"), recursive=True))[-1]
        size = a.sizes[0]
        nf = a.frames[0] if a.frames else 1
        memory = {}
        rows = layer_table(lab, size, size, sd, nf, precision, memory)
        frames, ms = from_trace(path, rows)
        what = f"groups of {nf} frames (M, GFLOP and ms of the whole group)" if nf > 1 else "frames"
        lines = [f"per-layer kernel times at {size}x{size}, precision {a.precision}, median over {frames} {what} of {os.path.basename(path)}",
                 f"workspace: activations {memory['workspace'] / 1e6:.1f} MB ({memory['element']} bytes per element, {nf} frame(s)), "
                 f"split-K partials {memory['partials'] / 1e6:.1f} MB, weights {memory['weights'] / 1e6:.1f} MB",
                 f"{'layer':28s} {'M':>7s} {'N':>5s} {'K':>5s} {'GFLOP':>7s} {'tile':>8s} {'split':>5s} {'ms':>8s} {'TF/s':>7s} {'MB':>8s} {'GB/s':>7s}"]
        lines.append(f"{'pre_max + pre_apply':28s} {'':>7s} {'':>5s} {'':>5s} {'':>7s} {'':>8s} {'':>5s} {ms['pre_max + pre_apply']:8.4f}")
        tot_ms, tot_fl = ms["pre_max + pre_apply"], 0.0
        for r in rows:
            t = ms[r["name"]]
            tot_ms, tot_fl = tot_ms + t, tot_fl + r["flops"]
            lines.append(f"{r['name']:28s} {r['M']:7d} {r['N']:5d} {r['K']:5d} {r['flops'] / 1e9:7.3f} {r['tile']:>8s} {r['splits']:5d} "
                         f"{t:8.4f} {r['flops'] / t / 1e9:7.2f} {r['bytes'] / 1e6:8.2f} {r['bytes'] / t / 1e6:7.0f}")
        lines.append(f"{'sum of kernels':28s} {'':>7s} {'':>5s} {'':>5s} {tot_fl / 1e9:7.3f} {'':>8s} {'':>5s} {tot_ms:8.4f} "
                     f"{tot_fl / tot_ms / 1e9:7.2f}")
        text = "\n".join(lines)
        print(text)
        if a.out:
            name = (f"layers_{size}" if nf == 1 else f"layers_{size}_n{nf}") + tag + ".txt"
            open(os.path.join(a.out, name), "w").write(text + "\n")
        return
    pt.set_device(0)
    if a.frames:
        res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
               "precision": a.precision,
               "weights": "denoise_weights.random_state_dict(seed=1)", "frame": "Cornell box, 4 spp, n poses",
               "note": "ms_per_frame = median device-event window of one batch / n; n = 1 is pt_denoiser_enqueue", "sizes": {}}
        for s in a.sizes:
            entry = {}
            for n in a.frames:
                t = time_hip_frames(pt, s, s, sd, n, a.runs, a.warmup, precision)
                entry[str(n)] = {"batch_ms_median": float(np.median(t)), "batch_ms_min": float(t.min()),
                                 "ms_per_frame": float(np.median(t)) / n}
            one = entry.get("1", {}).get("ms_per_frame")
            for n, e in entry.items():
                if one:
                    e["speedup_vs_single"] = one / e["ms_per_frame"]
                print(f"{s}x{s} n={n}: batch {e['batch_ms_median']:.4f} ms, {e['ms_per_frame']:.4f} ms per frame"
                      + (f" ({e['speedup_vs_single']:.2f}x single)" if one else ""), flush=True)
            res["sizes"][str(s)] = entry
        if a.out:
            with open(os.path.join(a.out, f"frames_time{tag}.json"), "w") as f:
                json.dump(res, f, indent=1)
        return
    res = {"device": pt.device_info()["name"], "fingerprint": pt.build_fingerprint(), "runs": a.runs, "warmup": a.warmup,
           "precision": a.precision,
           "weights": "denoise_weights.random_state_dict(seed=1)", "frame": "Cornell box, 4 spp, default camera", "sizes": {}}
    for s in a.sizes:
        rows = layer_table(lab, s, s, sd, 1, precision)
        flops = sum(r["flops"] for r in rows)
        t = time_hip(pt, s, s, sd, a.runs, a.warmup, precision)
        entry = {"gflop": flops / 1e9, "hip_ms": {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())},
                 "hip_tflops": flops / np.median(t) / 1e9, "floor_ms_at_fp32_mfma_peak": flops / (FLOOR_TFS * 1e9)}
        if not a.no_torch:
            tt = time_torch(s, s, sd, max(a.runs // 4, 20), 5)
            entry["torch_fp32_ms"] = {"median": float(np.median(tt)), "min": float(tt.min())}
        res["sizes"][str(s)] = entry
        print(f"{s}x{s}: {flops / 1e9:.2f} GFLOP, HIP median {entry['hip_ms']['median']:.4f} ms ({entry['hip_tflops']:.1f} TF/s), "
              f"floor {entry['floor_ms_at_fp32_mfma_peak']:.4f} ms"
              + (f", torch fp32 {entry['torch_fp32_ms']['median']:.4f} ms" if "torch_fp32_ms" in entry else ""), flush=True)
    if a.out:
        with open(os.path.join(a.out, f"denoise_time{tag}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
