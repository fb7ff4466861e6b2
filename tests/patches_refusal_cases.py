"""Every refusal of the training-patch stage (pt_patches_*) as flat lists of (case id, entry point, arguments, the word its
message must hold), built only from the public ABI through pt.lib: host_cases come before the device check
(tests/test_patches_host.py plays them without a GPU), live_cases are played on a live 8 x 8 session with patch 4 and
max_patches 2 (tests/test_patches_gpu.py); unprepared_cases on such a session before its first prepare."""
import ctypes

import numpy as np

W = H = 8
P, K = 4, 2
PT_EINVAL = -1

HOST_ENTRIES = {
    "pt_patches_create", "pt_patches_workspace_bytes", "pt_patches_prepare", "pt_patches_score", "pt_patches_result", "pt_patches_gather",
    "pt_patches_run_prepare", "pt_patches_run_score", "pt_patches_run_gather",
}


def _opts(pt, **changes):
    o = pt.PatchesOpts()
    pt.lib.pt_patches_opts_default(ctypes.byref(o))
    for k, v in changes.items():
        setattr(o, k, v)
    return o


def corners(*pairs):
    """A host int32 array of (x, y) pairs and its address (the array must outlive the call: keep the first)."""
    a = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return a, a.ctypes.data


def host_cases(pt):
    """(id, entry, args, word); a create's last argument None stands for a fresh output handle."""
    c = [("create.null_out", "pt_patches_create", (64, 64, None, "NULL"), "null output")]

    def create(cid, word, w=64, h=64, **changes):
        c.append((f"create.{cid}", "pt_patches_create", (w, h, _opts(pt, **changes), None), word))

    create("width=0", "width", w=0)
    create("width=16385", "width", w=16385)
    create("height=0", "height", h=0)
    create("height=16385", "height", h=16385)
    create("size=8192x8192", "4096 x 4096", w=8192, h=8192)
    create("patch=0", "patch", patch=0)
    create("patch=-1", "patch", patch=-1)
    create("patch>width", "patch", w=32, patch=33)
    create("patch>height", "patch", h=32, patch=33)
    create("patch=1025", "patch", w=2048, h=2048, patch=1025)
    create("max_patches=0", "max_patches", max_patches=0)
    create("max_patches=65536", "max_patches", patch=1, max_patches=65536)
    create("pixels>2^26", "max_patches", w=1024, h=1024, patch=1024, max_patches=65)
    for k in range(2):
        r = [0, 0]
        r[k] = 5
        create(f"reserved[{k}]", f"reserved[{k}]", reserved=tuple(r))
    values = pt.PatchesValues()
    keep, xy = corners((0, 0))
    c += [
        ("workspace_bytes.null", "pt_patches_workspace_bytes", (None, None), "null session"),
        ("prepare.null", "pt_patches_prepare", (None, None, None), "null session"),
        ("run_prepare.null", "pt_patches_run_prepare", (None, None, None), "null session"),
        ("score.null", "pt_patches_score", (None, None, 1, xy, None), "null session"),
        ("run_score.null", "pt_patches_run_score", (None, None, 1, xy, None), "null session"),
        ("gather.null", "pt_patches_gather", (None, None, None, 14, 1, xy, None, None, None), "null session"),
        ("run_gather.null", "pt_patches_run_gather", (None, None, None, 14, 1, xy, None, None, None), "null session"),
        ("result.null", "pt_patches_result", (None, 0, ctypes.byref(values)), "null session"),
    ]
    c.append(("_keep", None, keep, None))  # (the corner array lives as long as the list)
    return c


def unprepared_cases(pt, session, train, gt, inputs, targets):
    """On a live session before its first prepare: valid arguments, refused for that alone."""
    S = session
    keep, xy = corners((0, 0), (4, 4))
    return [
        ("score.unprepared", "pt_patches_score", (S, train, 2, xy, None), "pt_patches_prepare"),
        ("run_score.unprepared", "pt_patches_run_score", (S, train, 2, xy, None), "pt_patches_prepare"),
        ("gather.unprepared", "pt_patches_gather", (S, train, gt, 14, 2, xy, inputs, targets, None), "pt_patches_prepare"),
        ("run_gather.unprepared", "pt_patches_run_gather", (S, train, gt, 14, 2, xy, inputs, targets, None), "pt_patches_prepare"),
        ("_keep", None, keep, None),
    ]


def live_cases(pt, session, train, gt, inputs, targets):
    """On a live, prepared 8 x 8 session with patch 4 and max_patches 2; train and gt are frames of 14 floats per pixel (gt has
    room for 64), inputs and targets hold two patches."""
    S = session
    c, keep = [], []

    def xy(*pairs):
        a, addr = corners(*pairs)
        keep.append(a)
        return addr

    good = xy((0, 0), (4, 4))
    bad = [("x=-1", xy((0, 0), (-1, 0)), "corners[1].x = -1"), ("x=W-P+1", xy((W - P + 1, 0)), f"corners[0].x = {W - P + 1}"),
           ("y=-1", xy((2, -1)), "corners[0].y = -1"), ("y=H-P+1", xy((0, 0), (4, H - P + 1)), f"corners[1].y = {H - P + 1}")]
    for call, tail in (("score", (None,)), ("run_score", (None,))):
        e = f"pt_patches_{call}"
        c += [(f"{call}.{cid}", e, (S, train, 1 if "[0]" in word else 2, addr) + tail, word) for cid, addr, word in bad]
        c += [
            (f"{call}.n=0", e, (S, train, 0, good) + tail, "n 0"),
            (f"{call}.n=3", e, (S, train, 3, good) + tail, "n 3"),
            (f"{call}.n=-1", e, (S, train, -1, good) + tail, "n -1"),
            (f"{call}.null_d_train", e, (S, None, 2, good) + tail, "null d_train"),
            (f"{call}.null_corners", e, (S, train, 2, None) + tail, "null corners"),
        ]
    for call in ("gather", "run_gather"):
        e = f"pt_patches_{call}"
        c += [(f"{call}.{cid}", e, (S, train, gt, 14, 1 if "[0]" in word else 2, addr, inputs, targets, None), word) for cid, addr, word in bad]
        c += [
            (f"{call}.n=0", e, (S, train, gt, 14, 0, good, inputs, targets, None), "n 0"),
            (f"{call}.n=3", e, (S, train, gt, 14, 3, good, inputs, targets, None), "n 3"),
            (f"{call}.null_d_train", e, (S, None, gt, 14, 2, good, inputs, targets, None), "null d_train"),
            (f"{call}.null_d_gt", e, (S, train, None, 14, 2, good, inputs, targets, None), "null d_gt"),
            (f"{call}.null_d_inputs", e, (S, train, gt, 14, 2, good, None, targets, None), "null d_inputs"),
            (f"{call}.null_corners", e, (S, train, gt, 14, 2, None, inputs, targets, None), "null corners"),
            (f"{call}.gt_pixel_stride=2", e, (S, train, gt, 2, 2, good, inputs, targets, None), "gt_pixel_stride 2"),
            (f"{call}.gt_pixel_stride=65", e, (S, train, gt, 65, 2, good, inputs, targets, None), "gt_pixel_stride 65"),
        ]
    values = ctypes.byref(pt.PatchesValues())
    c += [
        ("prepare.null_d_train", "pt_patches_prepare", (S, None, None), "null d_train"),
        ("run_prepare.null_d_train", "pt_patches_run_prepare", (S, None, None), "null d_train"),
        ("workspace_bytes.null_out", "pt_patches_workspace_bytes", (S, None), "null output"),
        ("result.null_out", "pt_patches_result", (S, 0, None), "null output"),
        ("result.patch_index=-1", "pt_patches_result", (S, -1, values), "patch_index"),
        ("result.patch_index=past", "pt_patches_result", (S, 2, values), "patch_index"),  # (after a score of two patches)
        ("_keep", None, keep, None),
    ]
    return c


def play(pt, cases):
    """Plays the cases; every one must return PT_EINVAL with a message holding its word.  -> number played."""
    played = 0
    for cid, entry, args, word in cases:
        if entry is None:
            continue
        handle = ctypes.c_void_p(0xdead)
        real = list(args)
        if entry == "pt_patches_create":
            real[2] = ctypes.byref(real[2]) if real[2] is not None else None
            real[3] = None if real[3] == "NULL" else ctypes.byref(handle)
        rc = getattr(pt.lib, entry)(*real)
        msg = pt.lib.pt_last_error().decode()
        assert rc == PT_EINVAL, (cid, rc, msg)
        assert word in msg and entry in msg, (cid, msg)
        if entry == "pt_patches_create" and real[3] is not None:
            assert handle.value is None, (cid, "a refused create leaves a null handle")
        played += 1
    return played
