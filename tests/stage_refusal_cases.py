"""Every refusal of the four post-process stages (pt_denoiser_*, pt_filter_*, pt_temporal_*, pt_tonemap_*) as a flat list of
(case id, entry point, arguments), built only from the public ABI through pt.lib.  tests/golden/stage_refusals.json holds what
each case returns, {case id: [code, message]} with any " (file:line)" suffix stripped; test_stage_refusals_host.py plays the
half that needs no device, test_stage_refusals_gpu.py the half on live 8 x 8 sessions.  A refused call launches nothing; the one
accepted call of the list (the filter takes samples 0 beside a count image) runs on valid, zeroed buffers.

Recording (the committed file was made with the library of the commit BEFORE the stages got their shared host scaffold):
    PT_LIB_OVERRIDE=<that build's libptcore.so> python tests/stage_refusal_cases.py out.json [--live]
--live adds the half on live sessions and needs a GPU; without it that half is taken over from the existing out.json."""
import contextlib
import ctypes
import json
import os
import re
import sys

W = H = 8                      # the live sessions' frames
PIXELS = W * H
FRAME, RGB = PIXELS * 14, PIXELS * 3   # the smallest strides
MAX_FRAMES = 2
NAN, INF = float("nan"), float("inf")


class Live:
    """Placeholder: the handle of the live session of a stage."""

    def __init__(self, stage):
        self.stage = stage


class Dev:
    """Placeholder: a zeroed device buffer ("frames": two frames of 64 floats per pixel, "out", "counts")."""

    def __init__(self, name):
        self.name = name


class NewHandle:
    """Placeholder: a fresh output handle for a create."""


DENOISER, FILTER, TEMPORAL, TONEMAP = Live("denoiser"), Live("filter"), Live("temporal"), Live("tonemap")
FRAMES, OUT, COUNTS = Dev("frames"), Dev("out"), Dev("counts")
HANDLE = NewHandle()

# the entry points each half must reach (the tests assert it, so an emptied list cannot pass)
HOST_ENTRIES = {
    "pt_denoiser_create", "pt_denoiser_create_opts", "pt_denoiser_precision", "pt_denoiser_reserve_frames", "pt_denoiser_enqueue",
    "pt_denoiser_denoise", "pt_denoiser_enqueue_frames", "pt_denoiser_denoise_frames",
    "pt_filter_create", "pt_filter_reserve_frames", "pt_filter_workspace_bytes", "pt_filter_enqueue", "pt_filter_run",
    "pt_filter_enqueue_frames", "pt_filter_run_frames",
    "pt_temporal_create", "pt_temporal_reset", "pt_temporal_workspace_bytes", "pt_temporal_camera", "pt_temporal_enqueue", "pt_temporal_run",
    "pt_temporal_enqueue_frames", "pt_temporal_run_frames",
    "pt_tonemap_create", "pt_tonemap_reset", "pt_tonemap_workspace_bytes", "pt_tonemap_reserve_frames", "pt_tonemap_enqueue", "pt_tonemap_run",
    "pt_tonemap_enqueue_frames", "pt_tonemap_run_frames", "pt_tonemap_exposure",
}
LIVE_ENTRIES = (HOST_ENTRIES - {"pt_denoiser_create", "pt_denoiser_create_opts", "pt_filter_create", "pt_temporal_create", "pt_tonemap_create",
                                "pt_temporal_reset", "pt_tonemap_reset", "pt_temporal_camera"})  # (a live reset refuses nothing)


def _opts(pt, struct, default, **changes):
    o = struct()
    getattr(pt.lib, default)(ctypes.byref(o))
    for k, v in changes.items():
        setattr(o, k, v)
    return ctypes.byref(o)


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


def host_cases(pt):
    """The refusals that come before the device check: PT_EINVAL with or without a GPU."""
    c = []

    def sizes(stage, create):
        for tag, w, h in (("width=0", 0, 64), ("width=16385", 16385, 64), ("height=-3", 64, -3), ("height=16385", 64, 16385),
                          ("size=8192x8192", 8192, 8192)):
            create(f"{stage}.create.{tag}", w, h)

    # ---- filter
    def fcreate(cid, w=64, h=64, **changes):
        c.append((cid, "pt_filter_create", (w, h, _opts(pt, pt.FilterOpts, "pt_filter_opts_default", **changes), HANDLE)))

    c.append(("filter.create.null_out", "pt_filter_create", (64, 64, None, None)))
    sizes("filter", fcreate)
    fcreate("filter.create.iterations=0", iterations=0)
    fcreate("filter.create.iterations=9", iterations=9)
    fcreate("filter.create.sigma_l=0", sigma_l=0.0)
    fcreate("filter.create.sigma_n=nan", sigma_n=NAN)
    fcreate("filter.create.sigma_a=inf", sigma_a=INF)
    fcreate("filter.create.sigma_z=-1", sigma_z=-1.0)
    fcreate("filter.create.max_frames=0", max_frames=0)
    fcreate("filter.create.max_frames=65536", max_frames=65536)
    fcreate("filter.create.pixels>2^26", 4096, 4096, max_frames=5)
    fcreate("filter.create.reserved[0]", reserved=(1, 0))
    fcreate("filter.create.reserved[1]", reserved=(0, 3))
    c += [
        ("filter.reserve_frames.null", "pt_filter_reserve_frames", (None, 2)),
        ("filter.workspace_bytes.null", "pt_filter_workspace_bytes", (None, None)),
        ("filter.enqueue.null", "pt_filter_enqueue", (None, None, None, 4, None, None)),
        ("filter.run.null", "pt_filter_run", (None, None, None, 4, None, None)),
        ("filter.enqueue_frames.null", "pt_filter_enqueue_frames", (None, 2, None, FRAME, None, RGB, 4, None)),
        ("filter.run_frames.null", "pt_filter_run_frames", (None, 2, None, FRAME, None, RGB, 4, None)),
    ]

    # ---- temporal
    def tcreate(cid, w=64, h=64, **changes):
        c.append((cid, "pt_temporal_create", (w, h, _opts(pt, pt.TemporalOpts, "pt_temporal_opts_default", **changes), HANDLE)))

    c.append(("temporal.create.null_out", "pt_temporal_create", (64, 64, None, None)))
    sizes("temporal", tcreate)
    tcreate("temporal.create.history_cap=0.5", history_cap=0.5)
    tcreate("temporal.create.history_cap=nan", history_cap=NAN)
    tcreate("temporal.create.depth_tol=0", depth_tol=0.0)
    tcreate("temporal.create.depth_tol=inf", depth_tol=INF)
    tcreate("temporal.create.normal_tol=1.5", normal_tol=1.5)
    tcreate("temporal.create.albedo_tol=0", albedo_tol=0.0)
    tcreate("temporal.create.albedo_tol=inf", albedo_tol=INF)
    tcreate("temporal.create.min_weight=0", min_weight=0.0)
    tcreate("temporal.create.min_weight=1.5", min_weight=1.5)
    tcreate("temporal.create.reserved", reserved=1)
    basis = [float(v) for v in pt.camera_basis(width=W, height=H)]
    P = _floats([0.0] * 9)
    c += [
        ("temporal.reset.null", "pt_temporal_reset", (None,)),
        ("temporal.workspace_bytes.null", "pt_temporal_workspace_bytes", (None, None)),
        ("temporal.camera.null_basis", "pt_temporal_camera", (None, P)),
        ("temporal.camera.null_out", "pt_temporal_camera", (_floats(basis), None)),
        ("temporal.camera.singular", "pt_temporal_camera", (_floats([0.0] * 12), P)),
        ("temporal.camera.not_a_parallelogram", "pt_temporal_camera", (_floats(basis[:9] + [basis[9] + 1.0] + basis[10:]), P)),
        ("temporal.enqueue.null", "pt_temporal_enqueue", (None, None, 4, None, None, None, None)),
        ("temporal.run.null", "pt_temporal_run", (None, None, 4, None, None, None, None)),
        ("temporal.enqueue_frames.null", "pt_temporal_enqueue_frames", (None, 2, None, FRAME, None, None, 4, None, None)),
        ("temporal.run_frames.null", "pt_temporal_run_frames", (None, 2, None, FRAME, None, None, 4, None, None)),
    ]

    # ---- tonemap
    def mcreate(cid, w=64, h=64, **changes):
        c.append((cid, "pt_tonemap_create", (w, h, _opts(pt, pt.TonemapOpts, "pt_tonemap_opts_default", **changes), HANDLE)))

    c.append(("tonemap.create.null_out", "pt_tonemap_create", (64, 64, None, None)))
    sizes("tonemap", mcreate)
    mcreate("tonemap.create.curve=-1", curve=-1)
    mcreate("tonemap.create.curve=3", curve=3)
    mcreate("tonemap.create.encode=2", encode=2)
    mcreate("tonemap.create.exposure=-1", exposure=-1.0)
    mcreate("tonemap.create.exposure=nan", exposure=NAN)
    mcreate("tonemap.create.key=0", key=0.0)
    mcreate("tonemap.create.key=inf", key=INF)
    mcreate("tonemap.create.white=0", white=0.0)
    mcreate("tonemap.create.adapt=0", adapt=0.0)
    mcreate("tonemap.create.adapt=1.5", adapt=1.5)
    mcreate("tonemap.create.max_frames=0", max_frames=0)
    mcreate("tonemap.create.max_frames=65536", max_frames=65536)
    mcreate("tonemap.create.pixels>2^26", 4096, 4096, max_frames=5)
    mcreate("tonemap.create.reserved[0]", reserved=(1, 0))
    mcreate("tonemap.create.reserved[1]", reserved=(0, 3))
    c += [
        ("tonemap.reset.null", "pt_tonemap_reset", (None,)),
        ("tonemap.workspace_bytes.null", "pt_tonemap_workspace_bytes", (None, None)),
        ("tonemap.reserve_frames.null", "pt_tonemap_reserve_frames", (None, 2)),
        ("tonemap.exposure.null", "pt_tonemap_exposure", (None, None)),
        ("tonemap.enqueue.null", "pt_tonemap_enqueue", (None, None, 14, None, None)),
        ("tonemap.run.null", "pt_tonemap_run", (None, None, 14, None, None)),
        ("tonemap.enqueue_frames.null", "pt_tonemap_enqueue_frames", (None, 2, None, FRAME, 14, None, PIXELS, None)),
        ("tonemap.run_frames.null", "pt_tonemap_run_frames", (None, 2, None, FRAME, 14, None, PIXELS, None)),
    ]

    # ---- denoiser (every refusal here comes before the weights are read: any bytes do)
    def dcreate(cid, w=16, h=16, blob=b"PTDN", **changes):
        reserved = changes.pop("reserved", {})
        o = pt.DenoiserOpts(precision=changes.pop("precision", 0), max_frames=changes.pop("max_frames", 1))
        for i, v in reserved.items():
            o.reserved[i] = v
        c.append((cid, "pt_denoiser_create_opts", (w, h, blob, len(blob), ctypes.byref(o), HANDLE)))

    c += [
        ("denoiser.create.null_out", "pt_denoiser_create", (16, 16, b"PTDN", 4, None)),
        ("denoiser.create_opts.null_out", "pt_denoiser_create_opts", (16, 16, b"PTDN", 4, ctypes.byref(pt.DenoiserOpts(max_frames=1)), None)),
        ("denoiser.create_opts.null_options", "pt_denoiser_create_opts", (16, 16, b"PTDN", 4, None, HANDLE)),
    ]
    dcreate("denoiser.create_opts.precision=2", precision=2)
    dcreate("denoiser.create_opts.precision=-1", precision=-1)
    dcreate("denoiser.create_opts.max_frames=0", max_frames=0)
    for i in range(6):
        dcreate(f"denoiser.create_opts.reserved[{i}]", reserved={i: 7})
    dcreate("denoiser.create_opts.width=0", w=0)
    dcreate("denoiser.create_opts.height=-3", h=-3)
    dcreate("denoiser.create_opts.size=8192x8192", w=8192, h=8192)
    dcreate("denoiser.create_opts.max_frames=65536", max_frames=65536)
    dcreate("denoiser.create_opts.pixels>2^26", w=4096, h=4096, max_frames=5)
    c += [
        ("denoiser.precision.null", "pt_denoiser_precision", (None, None)),
        ("denoiser.reserve_frames.null", "pt_denoiser_reserve_frames", (None, 2)),
        ("denoiser.enqueue.null", "pt_denoiser_enqueue", (None, None, None, None)),
        ("denoiser.denoise.null", "pt_denoiser_denoise", (None, None, None, None)),
        ("denoiser.enqueue_frames.null", "pt_denoiser_enqueue_frames", (None, 2, None, FRAME, None, RGB, None)),
        ("denoiser.denoise_frames.null", "pt_denoiser_denoise_frames", (None, 2, None, FRAME, None, RGB, None)),
    ]
    return c


def live_cases(pt):
    """The refusals of live 8 x 8 sessions with max_frames 2 (play() makes them: see live_sessions)."""
    c = []
    reserves = (("0", 0), ("65536", 65536), ("pixels>2^26", 2000000))

    # ---- filter: single (entry, d_frame, d_rgb, samples, d_counts, last), batched (entry, n, d_frames, stride, d_rgb, stride, samples, last)
    for call in ("enqueue", "run"):
        e, eb = f"pt_filter_{call}", f"pt_filter_{call}_frames"
        c += [
            (f"filter.{call}.null_d_frame", e, (FILTER, None, None, 4, None, None)),
            (f"filter.{call}.samples=0", e, (FILTER, FRAMES, None, 0, None, None)),
            (f"filter.{call}.samples=0.with_counts", e, (FILTER, FRAMES, None, 0, COUNTS, None)),  # accepted: the counts replace it
            (f"filter.{call}_frames.null_d_frames", eb, (FILTER, 2, None, FRAME, None, RGB, 4, None)),
            (f"filter.{call}_frames.n_frames=0", eb, (FILTER, 0, FRAMES, FRAME, None, RGB, 4, None)),
            (f"filter.{call}_frames.frame_stride", eb, (FILTER, 2, FRAMES, FRAME - 1, None, RGB, 4, None)),
            (f"filter.{call}_frames.rgb_stride", eb, (FILTER, 2, FRAMES, FRAME, OUT, RGB - 1, 4, None)),
            (f"filter.{call}_frames.samples=0", eb, (FILTER, 2, FRAMES, FRAME, None, RGB, 0, None)),
        ]
    c += [(f"filter.reserve_frames.{tag}", "pt_filter_reserve_frames", (FILTER, n)) for tag, n in reserves]
    c.append(("filter.workspace_bytes.null_out", "pt_filter_workspace_bytes", (FILTER, None)))

    # ---- denoiser: single (entry, d_frame, d_rgb, last), batched (entry, n, d_frames, stride, d_rgb, stride, last)
    for single, batched in (("enqueue", "enqueue_frames"), ("denoise", "denoise_frames")):
        e, eb = f"pt_denoiser_{single}", f"pt_denoiser_{batched}"
        c += [
            (f"denoiser.{single}.null_d_frame", e, (DENOISER, None, None, None)),
            (f"denoiser.{batched}.null_d_frames", eb, (DENOISER, 2, None, FRAME, None, RGB, None)),
            (f"denoiser.{batched}.n_frames=0", eb, (DENOISER, 0, FRAMES, FRAME, None, RGB, None)),
            (f"denoiser.{batched}.frame_stride", eb, (DENOISER, 2, FRAMES, FRAME - 1, None, RGB, None)),
            (f"denoiser.{batched}.rgb_stride", eb, (DENOISER, 2, FRAMES, FRAME, OUT, RGB - 1, None)),
        ]
    c += [(f"denoiser.reserve_frames.{tag}", "pt_denoiser_reserve_frames", (DENOISER, n)) for tag, n in reserves]
    c.append(("denoiser.precision.null_out", "pt_denoiser_precision", (DENOISER, None)))

    # ---- temporal: single (entry, d_frame, samples, basis, eye, d_counts, last),
    #      batched (entry, n, d_frames, stride, bases, eyes, samples, d_counts, last)
    basis = [float(v) for v in pt.camera_basis(width=W, height=H)]
    eye = [float(v) for v in pt.DEFAULT_EYE]
    B, E, B2, E2 = _floats(basis), _floats(eye), _floats(basis * 2), _floats(eye * 2)
    singular, skewed = [0.0] * 12, basis[:9] + [basis[9] + 1.0] + basis[10:]
    for call in ("enqueue", "run"):
        e, eb = f"pt_temporal_{call}", f"pt_temporal_{call}_frames"
        c += [
            (f"temporal.{call}.null_d_frame", e, (TEMPORAL, None, 4, B, E, None, None)),
            (f"temporal.{call}.samples=0", e, (TEMPORAL, FRAMES, 0, B, E, None, None)),
            (f"temporal.{call}.samples=0.with_counts", e, (TEMPORAL, FRAMES, 0, B, E, COUNTS, None)),
            (f"temporal.{call}.null_basis", e, (TEMPORAL, FRAMES, 4, None, E, None, None)),
            (f"temporal.{call}.null_eye", e, (TEMPORAL, FRAMES, 4, B, None, None, None)),
            (f"temporal.{call}.eye=nan", e, (TEMPORAL, FRAMES, 4, B, _floats([eye[0], NAN, eye[2]]), None, None)),
            (f"temporal.{call}.singular_basis", e, (TEMPORAL, FRAMES, 4, _floats(singular), E, None, None)),
            (f"temporal.{call}.not_a_parallelogram", e, (TEMPORAL, FRAMES, 4, _floats(skewed), E, None, None)),
            (f"temporal.{call}_frames.null_d_frames", eb, (TEMPORAL, 2, None, FRAME, B2, E2, 4, None, None)),
            (f"temporal.{call}_frames.n_frames=0", eb, (TEMPORAL, 0, FRAMES, FRAME, B2, E2, 4, None, None)),
            (f"temporal.{call}_frames.frame_stride", eb, (TEMPORAL, 2, FRAMES, FRAME - 1, B2, E2, 4, None, None)),
            (f"temporal.{call}_frames.samples=0", eb, (TEMPORAL, 2, FRAMES, FRAME, B2, E2, 0, None, None)),
            (f"temporal.{call}_frames.null_basis", eb, (TEMPORAL, 2, FRAMES, FRAME, None, E2, 4, None, None)),
            (f"temporal.{call}_frames.null_eye", eb, (TEMPORAL, 2, FRAMES, FRAME, B2, None, 4, None, None)),
            (f"temporal.{call}_frames.eye=inf.frame1", eb, (TEMPORAL, 2, FRAMES, FRAME, B2, _floats(eye + [eye[0], eye[1], INF]), 4, None, None)),
            (f"temporal.{call}_frames.singular_basis.frame1", eb, (TEMPORAL, 2, FRAMES, FRAME, _floats(basis + singular), E2, 4, None, None)),
            (f"temporal.{call}_frames.not_a_parallelogram.frame1", eb, (TEMPORAL, 2, FRAMES, FRAME, _floats(basis + skewed), E2, 4, None, None)),
        ]
    c.append(("temporal.workspace_bytes.null_out", "pt_temporal_workspace_bytes", (TEMPORAL, None)))

    # ---- tonemap: single (entry, d_src, pixel_stride, d_rgba8, last), batched (entry, n, d_src, stride, pixel_stride, d_rgba8, stride, last)
    for call in ("enqueue", "run"):
        e, eb = f"pt_tonemap_{call}", f"pt_tonemap_{call}_frames"
        c += [
            (f"tonemap.{call}.null_d_src", e, (TONEMAP, None, 14, OUT, None)),
            (f"tonemap.{call}.null_d_rgba8", e, (TONEMAP, FRAMES, 14, None, None)),
            (f"tonemap.{call}.pixel_stride=2", e, (TONEMAP, FRAMES, 2, OUT, None)),
            (f"tonemap.{call}.pixel_stride=65", e, (TONEMAP, FRAMES, 65, OUT, None)),
            (f"tonemap.{call}_frames.null_d_src", eb, (TONEMAP, 2, None, FRAME, 14, OUT, PIXELS, None)),
            (f"tonemap.{call}_frames.null_d_rgba8", eb, (TONEMAP, 2, FRAMES, FRAME, 14, None, PIXELS, None)),
            (f"tonemap.{call}_frames.n_frames=0", eb, (TONEMAP, 0, FRAMES, FRAME, 14, OUT, PIXELS, None)),
            (f"tonemap.{call}_frames.pixel_stride=2", eb, (TONEMAP, 2, FRAMES, FRAME, 2, OUT, PIXELS, None)),
            (f"tonemap.{call}_frames.pixel_stride=65", eb, (TONEMAP, 2, FRAMES, PIXELS * 65, 65, OUT, PIXELS, None)),
            (f"tonemap.{call}_frames.src_stride", eb, (TONEMAP, 2, FRAMES, FRAME - 1, 14, OUT, PIXELS, None)),
            (f"tonemap.{call}_frames.dst_stride", eb, (TONEMAP, 2, FRAMES, FRAME, 14, OUT, PIXELS - 1, None)),
        ]
    c += [(f"tonemap.reserve_frames.{tag}", "pt_tonemap_reserve_frames", (TONEMAP, n)) for tag, n in reserves]
    c += [("tonemap.workspace_bytes.null_out", "pt_tonemap_workspace_bytes", (TONEMAP, None)),
          ("tonemap.exposure.null_out", "pt_tonemap_exposure", (TONEMAP, None))]
    return c


@contextlib.contextmanager
def live_sessions(pt):
    """{placeholder name: handle or device pointer}: the four 8 x 8 sessions (max_frames 2; the denoiser on seeded test weights)
    and three zeroed device buffers; everything is released on exit."""
    from cuda_pathtrace_amd import denoise_weights

    made, bufs = [], []
    try:
        for cls, kw in ((pt.Denoiser, dict(weights=denoise_weights.random_state_dict(seed=3), max_frames=MAX_FRAMES)),
                        (pt.FeatureFilter, dict(max_frames=MAX_FRAMES)), (pt.Temporal, {}), (pt.Tonemap, dict(max_frames=MAX_FRAMES))):
            made.append(cls(W, H, **kw))
        env = dict(zip(("denoiser", "filter", "temporal", "tonemap"), (s.handle for s in made)))
        for name, nbytes in (("frames", MAX_FRAMES * PIXELS * 64 * 4), ("out", MAX_FRAMES * PIXELS * 16), ("counts", PIXELS * 4)):
            bufs.append(pt.DeviceBuffer(nbytes))
            pt.check(pt.lib.pt_memset(bufs[-1].ptr, 0, nbytes))
            env[name] = bufs[-1].ptr
        yield env
        pt.check(pt.lib.pt_device_synchronize())
    finally:
        for b in bufs:
            b.free()
        for s in made:
            s.destroy()


def play(pt, cases, env=None):
    """{case id: [code, message]} of `cases` on pt.lib; env: live_sessions' names for the placeholders."""
    out = {}
    for cid, entry, args in cases:
        handle = ctypes.c_void_p(0xdead)
        real = [env[a.stage] if isinstance(a, Live) else env[a.name] if isinstance(a, Dev) else ctypes.byref(handle) if a is HANDLE else a
                for a in args]
        rc = getattr(pt.lib, entry)(*real)
        assert cid not in out, cid
        out[cid] = [rc, re.sub(r" \([^()]*:\d+\)$", "", pt.lib.pt_last_error().decode()) if rc else ""]
        if HANDLE in args:
            assert handle.value is None, (cid, "a refused create leaves a null handle")
    return out


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge

    pt = ge.load_package()
    path, live = argv[0], "--live" in argv[1:]
    got = play(pt, host_cases(pt))
    if live:
        pt.set_device(0)
        with live_sessions(pt) as env:
            got.update(play(pt, live_cases(pt), env))
    elif os.path.exists(path):
        old = json.load(open(path))
        got.update({cid: old[cid] for cid, _, _ in live_cases(pt) if cid in old})
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(got[cid])}" for cid in sorted(got)) + "\n}\n")  # a line per case
    print(f"{len(got)} cases from {pt.LIB_PATH} ({pt.build_fingerprint()}) -> {path}")


if __name__ == "__main__":
    main(sys.argv[1:])
