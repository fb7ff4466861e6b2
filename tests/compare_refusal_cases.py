"""Every refusal of the comparison stage (pt_compare_*) as flat lists of (case id, entry point, arguments, the word its message
must hold), built only from the public ABI through pt.lib: host_cases come before the device check (tests/test_compare_host.py
plays them without a GPU), live_cases are played on a live 8 x 8 session with max_frames 2 (tests/test_compare_gpu.py).  The
other four stages have their own list, tests/stage_refusal_cases.py."""
import ctypes

W = H = 8
PIXELS = W * H
FRAME, RGB = PIXELS * 14, PIXELS * 3  # the smallest strides
PT_EINVAL = -1

HOST_ENTRIES = {
    "pt_compare_create", "pt_compare_workspace_bytes", "pt_compare_reserve_frames", "pt_compare_ssim_weights", "pt_compare_enqueue",
    "pt_compare_run", "pt_compare_enqueue_frames", "pt_compare_run_frames", "pt_compare_result",
}


def _opts(pt, **changes):
    o = pt.CompareOpts()
    pt.lib.pt_compare_opts_default(ctypes.byref(o))
    for k, v in changes.items():
        setattr(o, k, v)
    return o


def host_cases(pt):
    """(id, entry, args, word); a create's last argument None stands for a fresh output handle."""
    c = [("create.null_out", "pt_compare_create", (64, 64, None, "NULL"), "null output")]

    def create(cid, word, w=64, h=64, **changes):
        c.append((f"create.{cid}", "pt_compare_create", (w, h, _opts(pt, **changes), None), word))

    create("width=0", "width", w=0)
    create("width=16385", "width", w=16385)
    create("height=0", "height", h=0)
    create("height=16385", "height", h=16385)
    create("size=8192x8192", "4096 x 4096", w=8192, h=8192)
    create("max_frames=0", "max_frames", max_frames=0)
    create("max_frames=65536", "max_frames", max_frames=65536)
    create("pixels>2^26", "max_frames", w=4096, h=4096, max_frames=5)
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 5
        create(f"reserved[{k}]", f"reserved[{k}]", reserved=tuple(r))
    values = pt.CompareValues()
    c += [
        ("workspace_bytes.null", "pt_compare_workspace_bytes", (None, None), "null comparison"),
        ("reserve_frames.null", "pt_compare_reserve_frames", (None, 2), "null comparison"),
        ("ssim_weights.null", "pt_compare_ssim_weights", (None,), "null output"),
        ("enqueue.null", "pt_compare_enqueue", (None, None, 14, None, 14, None, None), "null comparison"),
        ("run.null", "pt_compare_run", (None, None, 14, None, 14, None, None), "null comparison"),
        ("enqueue_frames.null", "pt_compare_enqueue_frames", (None, 2, None, FRAME, 14, None, FRAME, 14, None, RGB, None), "null comparison"),
        ("run_frames.null", "pt_compare_run_frames", (None, 2, None, FRAME, 14, None, FRAME, 14, None, RGB, None), "null comparison"),
        ("result.null", "pt_compare_result", (None, 0, ctypes.byref(values)), "null comparison"),
    ]
    return c


def live_cases(pt, session, img, ref, out):
    """On a live 8 x 8 session with max_frames 2; img and ref hold two frames of 64 floats per pixel, out two maps."""
    S = session
    c = []
    for call in ("enqueue", "run"):
        e, eb = f"pt_compare_{call}", f"pt_compare_{call}_frames"
        c += [
            (f"{call}.null_d_img", e, (S, None, 14, ref, 14, out, None), "null d_img"),
            (f"{call}.null_d_ref", e, (S, img, 14, None, 14, out, None), "null d_ref"),
            (f"{call}.img_pixel_stride=2", e, (S, img, 2, ref, 14, out, None), "img_pixel_stride"),
            (f"{call}.img_pixel_stride=65", e, (S, img, 65, ref, 14, out, None), "img_pixel_stride"),
            (f"{call}.ref_pixel_stride=2", e, (S, img, 14, ref, 2, out, None), "ref_pixel_stride"),
            (f"{call}.ref_pixel_stride=65", e, (S, img, 14, ref, 65, out, None), "ref_pixel_stride"),
            (f"{call}_frames.null_d_img", eb, (S, 2, None, FRAME, 14, ref, FRAME, 14, out, RGB, None), "null d_img"),
            (f"{call}_frames.null_d_ref", eb, (S, 2, img, FRAME, 14, None, FRAME, 14, out, RGB, None), "null d_ref"),
            (f"{call}_frames.n_frames=0", eb, (S, 0, img, FRAME, 14, ref, FRAME, 14, out, RGB, None), "n_frames"),
            (f"{call}_frames.n_frames=-1", eb, (S, -1, img, FRAME, 14, ref, FRAME, 14, out, RGB, None), "n_frames"),
            (f"{call}_frames.img_pixel_stride=2", eb, (S, 2, img, FRAME, 2, ref, FRAME, 14, out, RGB, None), "img_pixel_stride"),
            (f"{call}_frames.ref_pixel_stride=65", eb, (S, 2, img, FRAME, 14, ref, PIXELS * 65, 65, out, RGB, None), "ref_pixel_stride"),
            (f"{call}_frames.img_stride", eb, (S, 2, img, FRAME - 1, 14, ref, FRAME, 14, out, RGB, None), "img_stride_floats"),
            (f"{call}_frames.ref_stride", eb, (S, 2, img, FRAME, 14, ref, FRAME - 1, 14, out, RGB, None), "ref_stride_floats"),
            (f"{call}_frames.ref_stride=1", eb, (S, 2, img, FRAME, 14, ref, 1, 3, out, RGB, None), "ref_stride_floats"),
            (f"{call}_frames.map_stride", eb, (S, 2, img, FRAME, 14, ref, FRAME, 14, out, RGB - 1, None), "map_stride_floats"),
        ]
    values = ctypes.byref(pt.CompareValues())
    c += [
        ("reserve_frames.0", "pt_compare_reserve_frames", (S, 0), "max_frames"),
        ("reserve_frames.65536", "pt_compare_reserve_frames", (S, 65536), "max_frames"),
        ("reserve_frames.pixels>2^26", "pt_compare_reserve_frames", (S, 2000000), "max_frames"),
        ("workspace_bytes.null_out", "pt_compare_workspace_bytes", (S, None), "null output"),
        ("result.null_out", "pt_compare_result", (S, 0, None), "null output"),
        ("result.frame_index=-1", "pt_compare_result", (S, -1, values), "frame_index"),
        ("result.frame_index=past", "pt_compare_result", (S, 2, values), "frame_index"),  # (after a call of two frames)
    ]
    return c


def play(pt, cases):
    """Plays the cases; every one must return PT_EINVAL with a message holding its word.  -> number played."""
    for cid, entry, args, word in cases:
        handle = ctypes.c_void_p(0xdead)
        real = list(args)
        if entry == "pt_compare_create":
            real[2] = ctypes.byref(real[2]) if real[2] is not None else None
            real[3] = None if real[3] == "NULL" else ctypes.byref(handle)
        rc = getattr(pt.lib, entry)(*real)
        msg = pt.lib.pt_last_error().decode()
        assert rc == PT_EINVAL, (cid, rc, msg)
        assert word in msg and entry in msg, (cid, msg)
        if entry == "pt_compare_create" and real[3] is not None:
            assert handle.value is None, (cid, "a refused create leaves a null handle")
    return len(cases)
