"""The cases of tests/test_denoiser_groups_gpu.py: groups of more than one frame through single convolutions of the denoiser
(csrc/pt_denoise.hip), and for every convolution of a case the REASON it is there, expressed on the plan model
(tests/denoise_plan_model.py).  tests/test_denoiser_groups_host.py shows without a device that every reason holds and what
the table covers; the GPU test holds the library's conv_plan(g) to the same model before it runs a case, so a changed plan
rule fails loudly instead of blinding a case.

A reason is a word checked by `holds(reason, row, precision, group)` on one row of plan(width, height, precision, group);
"a|b" means a in float32 and b in half.  A case lists reasons as (convolution or "*" = every convolution of the case, word).

What the rule cannot produce, and the table therefore does not hold (the host test asserts both):
  * a split head in half mode: the head has 18 chunks of K and a half slice is at least 16, so nchunks // min_chunks = 1;
  * a 256x32 tile with split-K in half mode, and in either mode with the lateral epilogue, inside the memory limit below: the
    32-column layers that split at all are the 1x1 laterals over 256 or more channels, on maps so small that 256 tiles of them
    need thousands of frames and gigabytes of partial sums (LEFT_OUT)."""
import numpy as np

import denoise_plan_model as P

MEMORY_LIMIT = 1 << 30  # bytes of activations + split-K partials of one denoiser in these tests
ALL = None
BOTH = ("float32", "half")
TILES = {(256, 32), (128, 64), (128, 128), (128, 32), (64, 64)}
WIDE = {(256, 32), (128, 64), (128, 128)}


def holds(reason, c, precision, g):
    """Whether `reason` holds for row c of plan(w, h, precision, g)."""
    if "|" in reason:
        key, _, vals = reason.partition("=")
        a, b = vals.split("|")
        reason = f"{key}={a if precision == 'float32' else b}"
    ih, iw, _ = c["in_shape"]
    if reason.startswith("tile="):
        return f"{c['bm']}x{c['bn']}" == reason[5:]
    if reason.startswith("splits="):
        return c["splits"] == int(reason[7:])
    return {
        "frames": g > 1 and c["M"] == g * c["out_hw"],
        "ragged": c["M"] % c["bm"] != 0,  # the last tile has rows past M
        "border_in_block": g > 1 and c["out_hw"] % 32 != 0,  # a frame ends inside a 32-row MFMA block
        "three_frames_in_tile": min(c["bm"], c["M"]) > 2 * c["out_hw"],
        "row_is_frame": c["out_hw"] == 1 and g > 1,
        "short_last_slice": c["splits"] > 1 and c["nchunks"] % c["chunks_per_split"] != 0,
        "split": c["splits"] > 1,
        "unsplit": c["splits"] == 1,
        "affine": c["epi"] == P.EPI_ACT,
        "lateral": c["epi"] == P.EPI_LAT,
        "head": c["epi"] == P.EPI_RGB,
        "residual": c["res"] >= 0,
        "two_outputs": c["out1"] >= 0,
        "window3_stride1": (c["ks"], c["stride"]) == (3, 1),
        "stride2_odd_h": c["stride"] == 2 and ih % 2 == 1 and ih > 1,
        "stride2_odd_w": c["stride"] == 2 and iw % 2 == 1 and iw > 1,
        "window_mostly_padding": c["ks"] == 3 and (ih, iw) == (1, 1),  # eight of nine taps are padding, next to other frames
        "up_h==1": c["up_shape"] is not None and c["up_shape"][0] == 1 and c["out_h"] > 1,
        "up_w==1": c["up_shape"] is not None and c["up_shape"][1] == 1 and c["out_w"] > 1,
    }[reason]


def _ragged(w, h):
    """37 x 29 and 29 x 37: frame borders inside a 32-row block at every level, odd strides, one-row / one-column coarse maps."""
    one, other = ("up_h==1", "up_w==1") if w > h else ("up_w==1", "up_h==1")
    return [("*", "frames"), ("*", "border_in_block"), ("*", "ragged"),
            ("block1.conv1+res_conv", "stride2_odd_h"), ("block1.conv1+res_conv", "stride2_odd_w"),
            ("block2.conv1+res_conv", "stride2_odd_h"), ("block2.conv1+res_conv", "stride2_odd_w"),
            ("block4.conv1+res_conv", "stride2_odd_w" if w > h else "stride2_odd_h"),
            ("backwards_10", "stride2_odd_h"), ("backwards_10", "stride2_odd_w"),
            ("lat_3", one), ("lat_3", "lateral"), ("lat_5", other),  # (lat_5 is one row of two pixels over a 1 x 1 map)
            ("lat_5", "split"), ("lat_5", "lateral"), ("lat_4", "splits=2|1"), ("lat_6", "split"), ("lat_6", "affine"),
            ("rgb_conv", "head"), ("rgb_conv", "splits=2|1"), ("rgb_conv", "tile=128x32"),
            ("block1.conv1+res_conv", "tile=64x64"), ("block2.conv2", "split"), ("block2.conv2", "tile=64x64")]


BLOCK5 = ("block5.conv1+res_conv", "block5.conv2")
SHORT = [(n, r) for n in BLOCK5 for r in ("frames", "short_last_slice", "tile=64x64", "border_in_block")]

# (width, height, groups, convolutions or ALL, precisions, [(convolution or "*", reason)])
CASES = [
    (37, 29, (2, 3), ALL, BOTH, _ragged(37, 29)),
    (29, 37, (2, 3), ALL, BOTH, _ragged(29, 37)),
    (7, 5, (3, 5), ALL, BOTH,
     [("*", "frames"), ("*", "three_frames_in_tile"), ("*", "border_in_block")]
     + [(n, "window_mostly_padding") for n in ("block3.conv2", "block4.conv1+res_conv", "block4.conv2", "block5.conv1+res_conv",
                                               "block5.conv2", "block6.conv1+res_conv", "block6.conv2", "backwards_65",
                                               "backwards_54", "backwards_43")]),
    (1, 1, (300,), ALL, BOTH, [("*", "frames"), ("*", "row_is_frame"), ("*", "ragged"), ("*", "three_frames_in_tile")]),
    (37, 29, (61,), ("block1.conv1+res_conv", "lat_0", "rgb_conv"), BOTH,
     [("*", "frames"), ("*", "ragged"), ("*", "border_in_block"),
      ("block1.conv1+res_conv", "tile=128x64"), ("block1.conv1+res_conv", "unsplit"), ("block1.conv1+res_conv", "two_outputs"),
      ("lat_0", "tile=256x32"), ("lat_0", "lateral"), ("lat_0", "unsplit"),
      ("rgb_conv", "tile=256x32"), ("rgb_conv", "head"), ("rgb_conv", "splits=2|1")]),
    (37, 29, (240,), ("block1.conv2", "block2.conv2", "lat_1"), BOTH,
     [("*", "frames"), ("block1.conv2", "tile=256x32"), ("block1.conv2", "window3_stride1"), ("block1.conv2", "residual"),
      ("block1.conv2", "splits=2|1"), ("block1.conv2", "ragged"), ("block1.conv2", "border_in_block"),
      ("block2.conv2", "tile=128x64"), ("block2.conv2", "splits=4|2"), ("block2.conv2", "residual"),
      ("lat_1", "tile=256x32"), ("lat_1", "lateral"), ("lat_1", "ragged")]),
    (37, 29, (416,), ("block2.conv1+res_conv",), BOTH,
     [("*", "frames"), ("*", "tile=128x128"), ("*", "two_outputs"), ("*", "splits=2|1"), ("*", "border_in_block")]),
    (37, 29, (816,), ("block3.conv1+res_conv",), BOTH,
     [("*", "frames"), ("*", "tile=128x128"), ("*", "two_outputs"), ("*", "splits=4|2"), ("*", "ragged"), ("*", "border_in_block")]),
    (353, 321, (2,), BLOCK5, ("float32",), SHORT),
    (513, 481, (2,), BLOCK5, ("half",), SHORT),
    # the float32 head is unsplit only from 256 tiles of one frame up
    (259, 253, (2,), ("rgb_conv",), ("float32",),
     [("*", "frames"), ("*", "head"), ("*", "unsplit"), ("*", "tile=256x32"), ("*", "ragged"), ("*", "border_in_block")]),
]

# pairings of a wide tile with split-K that the rule can produce but that need more memory than MEMORY_LIMIT: what -> why.
# The host test shows that nothing else is missing.
LEFT_OUT = {
    "256x32 split, lateral epilogue": "first at about 11 000 frames of 37 x 29 (lat_4 in float32), several GB of workspace",
}

PRE_CASES = [(37, 29), (300, 70)]  # pre-processing of groups: sizes; groups, strides and modes are the GPU test's
PRE_GROUPS = (3, 61)
END_TO_END = (37, 29, 816)  # enqueue_frames against the loop of single enqueues, product library


def params():
    """[(precision, width, height, group, names, reasons)] of every run of the GPU test."""
    return [(p, w, h, g, names, reasons) for w, h, groups, names, precs, reasons in CASES for g in groups for p in precs]


def rows_of(w, h, precision, g, names):
    """[(index, plan row)] of the case's convolutions, in execution order."""
    plan = P.plan(w, h, precision, g)
    rows = [(i, c) for i, c in enumerate(plan) if names is None or c["name"] in names]
    assert names is None or [c["name"] for _, c in rows] == list(names), [c["name"] for _, c in rows]
    return rows


def failed_reasons(w, h, precision, g, names, reasons):
    """The (convolution, reason) pairs of a case that do NOT hold on the model's plan."""
    rows = rows_of(w, h, precision, g, names)
    by = {c["name"]: c for _, c in rows}
    bad = []
    for name, reason in reasons:
        for n in (list(by) if name == "*" else [name]):
            if n not in by or not holds(reason, by[n], precision, g):
                bad.append((n, reason))
    return bad


# ---- inputs and the float64 reference of a case (shared by the host and the GPU test: the same seeds, the same numbers) -------

def seed_of(w, h, g):
    return 1000003 * g + 1000 * w + h


def alphabet(half):
    """The activations' alphabet of tests/test_denoiser_exact_gpu.py."""
    return np.array([-1, 0, 0, 1] if half else [-2, -1, 0, 1, 1, 2], dtype=np.float32)


def conv_inputs(rs, c, g, w, h, half):
    """Random inputs of convolution row c for a group of g frames, every frame different: {"x", "res", "up", "x0"} (None where
    the layer reads none), each [g][rows][cols][channels] float32.  Small integers where a sum must be exact; the coarse map and
    the albedo are arbitrary values that fp16 holds exactly, so both modes read the same numbers."""
    d = {"x": rs.choice(alphabet(half), size=(g,) + c["in_shape"]), "res": None, "up": None, "x0": None}
    if c["res"] >= 0:
        d["res"] = rs.integers(-3, 4, size=(g, c["out_h"], c["out_w"], c["N"])).astype(np.float32)
    if c["up"] >= 0:
        d["up"] = rs.normal(0.0, 8.0, (g,) + c["up_shape"]).astype(np.float16).astype(np.float32)
    if c["epi"] == P.EPI_RGB:
        d["x0"] = np.zeros((g, h, w, P.C["XC"]), np.float32)
        d["x0"][..., 6:9] = rs.uniform(0.0, 1.0, (g, h, w, 3)).astype(np.float16).astype(np.float32)
    return d


def conv_ref64_frames(x, wgt, stride, ks):
    """_conv_ref64 of tests/test_denoiser_gpu.py for every frame of x [g][rows][cols][cin], stacked: float64, no bias."""
    import torch
    import torch.nn.functional as F

    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    y = F.conv2d(xt, torch.from_numpy(np.asarray(wgt, dtype=np.float64)), stride=stride, padding=ks // 2)
    return y.permute(0, 2, 3, 1).numpy()


def conv_reference(dw, sdi, c, d, half):
    """The stored outputs of convolution row c on inputs d, [g][rows][cols][columns] per output, from the float64 reference of
    each frame.  The exactness preconditions are asserted here: every accumulation an integer below 2^24 - 2^12; the float64
    affine exact and, in half mode, every stored affine output an integer of magnitude <= 2048 (_affine_ref); every lateral
    reference finite and below 65504."""
    import denoise_exact_model as EM
    from test_denoiser_exact_gpu import _affine_ref
    from test_denoiser_gpu import _pad_input_weight, _torch_names

    refs = []
    col = 0
    for tname, bn in _torch_names(c["name"]):
        wgt = _pad_input_weight(sdi[tname + ".weight"], c["cin"])
        acc = conv_ref64_frames(d["x"], wgt, c["stride"], c["ks"])
        assert np.array_equal(acc, np.round(acc)) and np.abs(acc).max() < 2 ** 24 - 2 ** 12, c["name"]  # exact in any order
        if c["epi"] == P.EPI_ACT:
            res = d["res"][..., col:col + acc.shape[-1]] if d["res"] is not None and col == 0 else None
            ref = _affine_ref(acc, sdi, dw, tname, bn, res, half)
        elif c["epi"] == P.EPI_LAT:
            a32 = EM.f32_exact(acc)
            ref = np.stack([EM.lateral(a32[f], sdi[tname + ".bias"], d["up"][f], half) for f in range(acc.shape[0])])
            assert np.isfinite(ref).all() and np.abs(ref).max() < 65504.0, c["name"]
        else:
            ref = EM.head(EM.f32_exact(acc), sdi[tname + ".bias"], d["x0"][..., 6:9])
        refs.append(ref)
        col += acc.shape[-1]
    return refs


def integer_weights(dw, precision):
    """(integer state_dict, its PTDN bytes) of tests/test_denoiser_exact_gpu.py for a precision."""
    from test_denoiser_exact_gpu import _weights

    return _weights(dw, precision)
