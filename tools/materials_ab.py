#!/usr/bin/env python3
"""Kernel time of the materials kernel (PT_VARIANT_MATERIALS, csrc/pt_materials.hip) with the package found in a given directory:
the reference's box at 1024 x 1024 x 64 spp, 5 bounces, an all-diffuse table and SMALLPT_MATERIALS alternating round by round, 3
warm-up and 15 timed rounds, both generators.  Prints ONE JSON line: per arm the median, smallest and largest kernel ms of
pt_renderer_render and a checksum (xor of all words) of the last frame.

For comparing two builds of the library -- this commit's and another's -- run it once per build, in turn, several times:

    python tools/materials_ab.py cuda-pathtrace_amd this >> ab.jsonl
    python tools/materials_ab.py /path/to/other/cuda-pathtrace_amd parent >> ab.jsonl     # a directory holding that commit's
                                                                                          # __init__.py, denoise_weights.py and libptcore.so
profiles/lights/v101_parent_vs_this.jsonl is three such pairs."""
import importlib.util
import json
import os
import sys

import numpy as np


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    pkg, label = os.path.abspath(sys.argv[1]), sys.argv[2]
    spec = importlib.util.spec_from_file_location("ptpkg_ab", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    pt = importlib.util.module_from_spec(spec)
    sys.modules["ptpkg_ab"] = pt
    spec.loader.exec_module(pt)
    if pt.device_count() < 1:
        raise SystemExit("materials_ab: no HIP device (a time is measured on the GPU or not at all)")
    pt.set_device(0)
    size, spp = 1024, 64
    d_scene, n = pt.upload_scene(pt.scene_cornell())
    basis = pt.camera_basis(width=size, height=size)
    out = {"label": label, "fingerprint": pt.build_fingerprint()}
    for rng_name, rng in (("xorwow", pt.RNG_XORWOW), ("philox", pt.RNG_PHILOX)):
        arms = {}
        for name, table in (("all_diffuse", [(0, 0.0)] * 9), ("smallpt", pt.SMALLPT_MATERIALS)):
            r = pt.Renderer(size, size, spp, rng_mode=rng, persist_rng=False)
            r.set_materials(table)
            assert r.kernel_info(n)["variant"] == pt.VARIANT_MATERIALS
            arms[name] = (r, pt.DeviceBuffer(r.tile_floats * 4), [])
        for k in range(3 + 15):
            for name, (r, d_out, ms) in arms.items():
                t = r.render(d_out.ptr, d_scene.ptr, n, basis)
                if k >= 3:
                    ms.append(t)
        for name, (r, d_out, ms) in arms.items():
            frame = d_out.download(np.float32, (size, size, 14))
            out[f"{rng_name}/{name}"] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)),
                                         "frame_crc": int(np.bitwise_xor.reduce(frame.view(np.uint32).reshape(-1)))}
            d_out.free()
            r.destroy()
    d_scene.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
