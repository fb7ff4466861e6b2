"""Every convolution of the denoiser's plan, one at a time through the lab hooks, bit for bit against float64 at ragged,
non-square sizes, in both precisions (csrc/pt_denoise.hip: conv_kernel's five tile shapes, two main loops, split-K and three
epilogues).  Integer activations and weights make every accumulation exact; the affine epilogue is then exact in float64
and rounded once, and the lateral and head epilogues are restated in the kernel's own float32 arithmetic
(tests/denoise_exact_model.py, held to float64 by tests/test_denoiser_exact_host.py), so at NO size is anything tolerated.

Each case asserts, from the library's own plan (convs(), conv_plan(1)) and layer table, the reason it is there -- a ragged
last tile on a wide tile shape, a map of one row under the upsample, a short last K slice -- so that a change of the plan
rule makes the case fail instead of leaving it blind.  DENOISER.md, "Tests"; profiles/denoise_exact/README.md."""
import numpy as np
import pytest

import denoise_exact_model as EM
from test_denoiser_gpu import _conv_ref64, _layer_outputs, _pad_input_weight, _torch_names, bits
from test_denoiser_half_gpu import _integer_state_dict

pytestmark = pytest.mark.gpu

ALL_TILES = {(256, 32), (128, 64), (128, 128), (128, 32), (64, 64)}
NARROW = {(128, 32), (64, 64)}
ALL_KINDS = {(3, 1, 0), (3, 2, 0), (1, 1, 0), (1, 1, 1), (3, 1, 2)}  # (ks, stride, epilogue): ACT 0, LAT 1, RGB 2
BLOCK2 = ["block1.conv2", "block2.conv1+res_conv", "block2.conv2"]
BLOCK5 = ["block5.conv1+res_conv", "block5.conv2"]
# (width, height, convolutions or None = all, precisions, what the case asserts about the plan)
CASES = [
    (37, 29, None, ("float32", "half"), "ragged"),
    (29, 37, None, ("float32", "half"), "ragged"),
    (7, 5, None, ("float32", "half"), "borders"),
    (2, 1, None, ("float32", "half"), "borders"),
    (1, 1, None, ("float32", "half"), "borders"),
    (259, 253, None, ("float32", "half"), "wide"),
    (727, 721, BLOCK2, ("float32", "half"), "square_tile"),
    (353, 321, BLOCK5, ("float32",), "short_slice"),
    (513, 481, BLOCK5, ("half",), "short_slice"),
]
PARAMS = [(p, w, h, names, why) for w, h, names, precs, why in CASES for p in precs]


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


_blobs = {}
_plans = {}  # (precision, w, h) -> [(name, kind, tile, splits)] of the convolutions the case runs


def _weights(dw, precision):
    """(integer state_dict, its PTDN bytes): random_state_dict(integer=True) for float32 (non-trivial batch norms, one fma
    rounding), the half test's scale-1 / integer-shift batch norms for half (every stored value an integer)."""
    if precision not in _blobs:
        sdi = _integer_state_dict(dw) if precision == "half" else dw.random_state_dict(seed=5, integer=True)
        _blobs[precision] = (sdi, dw.to_bytes(sdi))
    return _blobs[precision]


def _table(dn, names):
    """[(index, name, info + plan + shapes)] of the convolutions of a case, in execution order."""
    layers = dn.layers()
    plan = dn.conv_plan(1)
    out = []
    for ci, (name, info) in enumerate(dn.convs()):
        if names is not None and name not in names:
            continue
        t = dict(info)
        t.update(plan[ci])
        assert (t["bm"], t["bn"], t["splits"]) == (info["bm"], info["bn"], info["splits"]), name  # conv_plan(1) is convs()
        t["in_shape"] = layers[info["in"]][1]
        t["out_shape"] = layers[info["out0"]][1] if info["out0"] >= 0 else layers[0][1][:2] + (3,)
        t["up_shape"] = layers[info["up"]][1] if info["up"] >= 0 else None
        t["nchunks"] = info["ks"] * info["ks"] * t["in_shape"][2] // 16
        assert t["M"] == t["out_shape"][0] * t["out_shape"][1], name
        out.append((ci, name, t))
    assert names is None or [n for _, n, _ in out] == list(names), [n for _, n, _ in out]
    return out


def _assert_reason(why, w, h, table):
    """The property of the plan that the case exists for."""
    by = {name: t for _, name, t in table}
    ragged = {(t["bm"], t["bn"]) for t in by.values() if t["M"] % t["bm"] != 0}
    if why in ("ragged", "borders", "wide"):
        assert len(table) == 26, len(table)
    if why == "ragged":
        ups = [t for t in by.values() if t["up_shape"]]
        assert any(t["up_shape"][0] == 1 for t in ups) and any(t["up_shape"][1] == 1 for t in ups)
        one_row = [t for t in ups if t["out_shape"][0] == 1 and t["out_shape"][1] > 1]
        one_col = [t for t in ups if t["out_shape"][1] == 1 and t["out_shape"][0] > 1]
        assert (one_row if w > h else one_col), [t["out_shape"] for t in ups]
        assert all(t["M"] % 32 != 0 for t in by.values()), [t["M"] for t in by.values()]
        assert {t["out_shape"][:2] for t in by.values()} >= {(1, 1), (h, w)} and len({t["M"] for t in by.values()}) >= 6
    elif why == "borders":
        assert all(t["M"] <= 35 and (t["bm"], t["bn"]) in NARROW for t in by.values())
        assert sum(t["M"] == 1 for t in by.values()) >= 8  # 1 x 1 maps: a 3 x 3 window is eight taps of padding
    elif why == "wide":
        assert by["lat_0"]["M"] == by["rgb_conv"]["M"] == w * h and w * h % 256 != 0
        for name in ("lat_0", "rgb_conv"):
            assert (by[name]["bm"], by[name]["bn"]) == (256, 32), (name, by[name])
        t = by["block1.conv1+res_conv"]
        assert (t["bm"], t["bn"]) == (128, 64) and t["M"] % 128 != 0, t
        assert ragged >= {(256, 32), (128, 64)}, ragged
        assert sum(t["stride"] == 2 and t["in_shape"][0] % 2 == 1 for t in by.values()) >= 2  # strides over an odd height
        assert sum(t["stride"] == 2 and t["in_shape"][1] % 2 == 1 for t in by.values()) >= 8  # and over an odd width
    elif why == "square_tile":
        t = by["block2.conv1+res_conv"]
        assert (t["bm"], t["bn"], t["N"]) == (128, 128, 128) and t["M"] % 128 != 0, t
        assert (by["block1.conv2"]["bm"], by["block1.conv2"]["bn"]) == (256, 32) and by["block1.conv2"]["M"] % 256 != 0
        assert (by["block2.conv2"]["bm"], by["block2.conv2"]["bn"]) == (128, 64) and by["block2.conv2"]["M"] % 128 != 0
    elif why == "short_slice":
        for name in BLOCK5:
            t = by[name]
            assert t["splits"] > 1 and t["nchunks"] % t["chunks_per_split"] != 0, (name, t)  # the last slice is short
    else:
        raise AssertionError(why)


def _affine_ref(acc, sdi, dw, tname, bn, res, half):
    """EPI_ACT from the exact accumulation: relu(acc + bias), the folded batch norm as ONE rounding (the kernel's fma: the
    float64 product and sum are shown to be exact, so the conversion is that rounding), + residual in float32, stored."""
    v = np.maximum(acc + sdi[tname + ".bias"].astype(np.float64), 0.0)
    if bn:
        s, t = (a.astype(np.float64) for a in dw.fold_bn(sdi, bn))
        p = v * s  # < 2^24 times a float32: exact
        r = p + t
        tt = r - p
        assert np.all((p - (r - tt)) + (t - tt) == 0.0), "the float64 affine is not exact"  # two-sum: no rounding error
        v = r
    ref = v.astype(np.float32)
    if res is not None:
        ref = ref + res
    if half:
        assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() <= 2048, float(np.abs(ref).max())
    return EM.to_stored(ref, half)


def _run_case(lab, dw, precision, w, h, names, why, capsys):
    half = precision == "half"
    sdi, blob = _weights(dw, precision)
    rs = np.random.default_rng(1000 * w + h)
    alphabet = np.array([-1, 0, 0, 1] if half else [-2, -1, 0, 1, 1, 2], dtype=np.float32)
    dn = lab.Denoiser(w, h, blob, precision=precision)
    d_rgb = lab.DeviceBuffer(w * h * 12)
    compared = differing = 0
    try:
        assert dn.precision == precision
        table = _table(dn, names)
        _plans[(precision, w, h)] = [(n, (t["ks"], t["stride"], t["epi"]), (t["bm"], t["bn"]), t["splits"]) for _, n, t in table]
        _assert_reason(why, w, h, table)
        for ci, name, t in table:
            x = rs.choice(alphabet, size=t["in_shape"])
            dn.set_activation(t["in"], x)
            res = up = alb = None
            if t["res"] >= 0:
                res = rs.integers(-3, 4, size=t["out_shape"]).astype(np.float32)
                dn.set_activation(t["res"], res)
            if t["up"] >= 0:  # arbitrary values that fp16 holds exactly: both modes read the same numbers
                up = rs.normal(0.0, 8.0, t["up_shape"]).astype(np.float16).astype(np.float32)
                dn.set_activation(t["up"], up)
            if t["epi"] == 2:
                x0 = np.zeros((h, w, 16), np.float32)
                x0[..., 6:9] = rs.uniform(0.0, 1.0, (h, w, 3)).astype(np.float16).astype(np.float32)
                dn.set_activation(0, x0)
                alb = x0[..., 6:9]
            dn.run_conv(ci, d_rgb.ptr)
            got = [d_rgb.download(np.float32, (h, w, 3))] if t["out0"] < 0 else _layer_outputs(dn, ci, t)
            parts = _torch_names(name)
            assert len(got) == len(parts), name
            for g, (tname, bn) in zip(got, parts):
                wgt = _pad_input_weight(sdi[tname + ".weight"], t["in_shape"][2])
                acc = _conv_ref64(x, wgt, t["stride"], t["ks"])
                assert np.array_equal(acc, np.round(acc)) and np.abs(acc).max() < 2 ** 24 - 2 ** 12, name  # exact in any order
                if t["epi"] == 0:
                    ref = _affine_ref(acc, sdi, dw, tname, bn, res, half)
                elif t["epi"] == 1:
                    ref = EM.lateral(EM.f32_exact(acc), sdi[tname + ".bias"], up, half)
                    assert np.isfinite(ref).all() and np.abs(ref).max() < 65504.0
                else:
                    ref = EM.head(EM.f32_exact(acc), sdi[tname + ".bias"], alb)
                assert g.shape == ref.shape, (name, g.shape, ref.shape)
                bad = np.argwhere(bits(g) != bits(ref))
                compared += g.size
                differing += len(bad)
                assert len(bad) == 0, (f"{precision} {w}x{h} {name} ({tname}, tile {t['bm']}x{t['bn']}, {t['splits']} slices of "
                                       f"{t['chunks_per_split']} of {t['nchunks']} chunks): {len(bad)} of {g.size} differ, first "
                                       + "; ".join(f"{b.tolist()} got {g[tuple(b)]!r} want {ref[tuple(b)]!r}" for b in bad[:4]))
    finally:
        d_rgb.free()
        dn.destroy()
    with capsys.disabled():
        tiles = sorted({(t["bm"], t["bn"]) for _, _, t in table})
        short = [f"{n} {t['nchunks']} chunks in {t['splits']} slices of {t['chunks_per_split']}" for _, n, t in table
                 if t["nchunks"] % t["chunks_per_split"] != 0]
        print(f"\n{precision} {w}x{h}: {len(table)} convolutions, {compared} elements compared, {differing} differ; tiles {tiles}, "
              f"slices {sorted({t['splits'] for _, _, t in table})}" + (f"; short last slice: {', '.join(short)}" if short else ""))


@pytest.mark.parametrize("precision,w,h,names,why", PARAMS, ids=[f"{p}-{w}x{h}" for p, w, h, _, _ in PARAMS])
def test_every_convolution_is_exact_at_ragged_sizes(lab, gpu, dw, precision, w, h, names, why, capsys):
    """Each listed convolution of a width x height denoiser, run alone on small-integer inputs (and, for the lateral and head
    epilogues, arbitrary fp16-representable coarse maps and albedos): the stored output equals the reference bit for bit.
    Preconditions are asserted, not assumed: every accumulation an integer below 2^24, in half mode every stored affine output
    an integer of magnitude <= 2048, the float64 affine exact.  A mismatch names the layer, the count and the first elements."""
    _run_case(lab, dw, precision, w, h, names, why, capsys)


@pytest.mark.parametrize("precision", ["float32", "half"])
def test_the_cases_cover_every_tile_slicing_and_kind(lab, gpu, dw, precision):
    """Over the cases of this file, in each precision: all five tile shapes, split and unsplit layers, every (kernel size,
    stride, epilogue) kind.  Read from the plans of the cases (made here for a case that has not run in this session)."""
    tiles, kinds, split = set(), set(), set()
    for p, w, h, names, _ in PARAMS:
        if p != precision:
            continue
        if (p, w, h) not in _plans:
            dn = lab.Denoiser(w, h, _weights(dw, p)[1], precision=p)
            try:
                _plans[(p, w, h)] = [(n, (t["ks"], t["stride"], t["epi"]), (t["bm"], t["bn"]), t["splits"]) for _, n, t in _table(dn, names)]
            finally:
                dn.destroy()
        for _, kind, tile, splits in _plans[(p, w, h)]:
            tiles.add(tile)
            kinds.add(kind)
            split.add(splits > 1)
    assert tiles == ALL_TILES, tiles
    assert split == {True, False}, split
    assert kinds == ALL_KINDS, kinds
