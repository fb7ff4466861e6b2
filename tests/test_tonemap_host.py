"""CPU tests of the tone-mapping stage (pt_tonemap_*, DENOISER.md "Tone mapping"): the exported symbols, the C ABI's option
checks without a device, the host sRGB table against the model bit for bit, the model's encode against float64, its meter on
known answers and log-normal images, its curves on every input class, and the CLI's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tonemap_model as tm
from conftest import ROOT

PT_EINVAL = -1
SYMBOLS = ("pt_tonemap_opts_default", "pt_tonemap_create", "pt_tonemap_destroy", "pt_tonemap_reset", "pt_tonemap_workspace_bytes",
           "pt_tonemap_reserve_frames", "pt_tonemap_srgb_table", "pt_tonemap_enqueue", "pt_tonemap_run", "pt_tonemap_enqueue_frames",
           "pt_tonemap_run_frames", "pt_tonemap_exposure")
F = np.float32


# ---- 1, 2: the C ABI ------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays
    assert ctypes.sizeof(pt.TonemapOpts) == 36
    for name, value in (("PT_TONEMAP_CLAMP", tm.CLAMP), ("PT_TONEMAP_REINHARD", tm.REINHARD), ("PT_TONEMAP_ACES", tm.ACES),
                        ("PT_ENCODE_SRGB", tm.SRGB), ("PT_ENCODE_LINEAR", tm.LINEAR)):
        assert f"#define {name} {value}\n" in header, name
    assert (pt.TONEMAP_CURVES, pt.TONEMAP_ENCODES) == (tm.CURVES, tm.ENCODES)


def test_default_options(pt):
    o = pt.TonemapOpts(curve=9, exposure=-1.0, reserved=(7, 7))
    pt.lib.pt_tonemap_opts_default(ctypes.byref(o))
    assert (o.curve, o.encode, o.exposure, o.key, o.white, o.adapt, o.max_frames, tuple(o.reserved)) == (
        tm.ACES, tm.SRGB, 0.0, F(0.18), 4.0, 1.0, 1, (0, 0))
    assert tm.DEFAULTS == dict(curve=tm.ACES, encode=tm.SRGB, exposure=0.0, key=0.18, white=4.0, adapt=1.0, max_frames=1)


def _create(pt, width=64, height=64, **changes):
    o = pt.TonemapOpts()
    pt.lib.pt_tonemap_opts_default(ctypes.byref(o))
    for k, v in changes.items():
        setattr(o, k, v)
    h = ctypes.c_void_p(0xdead)
    rc = pt.lib.pt_tonemap_create(width, height, ctypes.byref(o), ctypes.byref(h))
    return rc, h.value, pt.lib.pt_last_error().decode()


@pytest.mark.parametrize("changes,word", [
    (dict(curve=-1), "curve"), (dict(curve=3), "curve"), (dict(encode=2), "encode"), (dict(encode=-1), "encode"),
    (dict(exposure=-1.0), "exposure"), (dict(exposure=float("inf")), "exposure"), (dict(exposure=float("nan")), "exposure"),
    (dict(key=0.0), "key"), (dict(key=float("inf")), "key"), (dict(key=float("nan")), "key"), (dict(key=-0.18), "key"),
    (dict(white=0.0), "white"), (dict(white=float("inf")), "white"), (dict(white=float("nan")), "white"), (dict(white=1e-30), "white"),
    (dict(adapt=0.0), "adapt"), (dict(adapt=1.5), "adapt"), (dict(adapt=float("nan")), "adapt"), (dict(adapt=-0.5), "adapt"),
    (dict(max_frames=0), "max_frames"), (dict(max_frames=65536), "max_frames"), (dict(width=4096, height=4096, max_frames=5), "max_frames"),
    (dict(reserved=(1, 0)), "reserved[0]"), (dict(reserved=(0, 3)), "reserved[1]"),
    (dict(width=0), "width 0 outside"), (dict(height=-3), "height -3 outside"), (dict(width=16385), "width 16385 outside"),
    (dict(width=8192, height=8192), "frame size 8192 x 8192"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_create_validates_every_option_before_a_device_is_touched(pt, changes, word):
    """PT_EINVAL naming the argument -- on a machine without a GPU too, where a valid create is PT_ENODEVICE / PT_EHIP."""
    rc, handle, msg = _create(pt, **changes)
    assert rc == PT_EINVAL and handle is None, (rc, msg)
    assert word in msg and "pt_tonemap_create" in msg, msg


def test_null_arguments_are_refused_without_a_device(pt):
    assert pt.lib.pt_tonemap_create(64, 64, None, None) == PT_EINVAL
    for call, word in [
        (lambda: pt.lib.pt_tonemap_reset(None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_enqueue(None, None, 14, None, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_run(None, None, 14, None, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_enqueue_frames(None, 2, None, 14, 14, None, 1, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_run_frames(None, 2, None, 14, 14, None, 1, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_workspace_bytes(None, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_reserve_frames(None, 2), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_exposure(None, None), "null tone mapper"),
        (lambda: pt.lib.pt_tonemap_srgb_table(None), "null output pointer"),
    ]:
        assert call() == PT_EINVAL
        assert word in pt.lib.pt_last_error().decode()
    assert pt.lib.pt_tonemap_destroy(None) == 0


def test_python_view_refuses_unknown_names_before_the_library(pt):
    for kw in (dict(curve="filmic"), dict(encode="rec709"), dict(exposure=0.0)):
        with pytest.raises(ValueError):
            pt.Tonemap(8, 8, **kw)


# ---- 3: the table ---------------------------------------------------------------------------------------------------

def test_srgb_table_equals_the_model_bit_for_bit_and_increases(pt):
    got, want = pt.tonemap_srgb_table(), tm.srgb_table()
    assert got.dtype == np.float32 and got.shape == (255,) and want.shape == (255,)
    assert np.array_equal(tm.bits(got), tm.bits(want))
    assert (np.diff(got) > 0).all() and got[0] > 0 and got[-1] < 1
    # known ends: code 1 begins at 0.5 / 255 / 12.92, code 255 at the inverse of 254.5 / 255
    assert got[0] == F(0.5 / 255 / 12.92) and got[-1] == F(((254.5 / 255 + 0.055) / 1.055) ** 2.4)


# ---- 4: encode against float64 --------------------------------------------------------------------------------------

def test_srgb_encode_is_the_correctly_rounded_code():
    """2 10^6 values y = inverse-OETF(u), u uniform in [0, 1): the table search equals floor(255 OETF(y) + 0.5) in float64
    wherever 255 OETF(y) is not within 1e-4 of a half-integer, and that band holds at most 0.1 % of the values."""
    rng = np.random.default_rng(20261019)
    y = tm.inverse_oetf(rng.random(2_000_000)).astype(np.float32)
    got = tm.encode(y, tm.SRGB).astype(np.int64)
    v = 255.0 * tm.oetf(y.astype(np.float64))
    want = np.floor(v + 0.5).astype(np.int64)
    band = np.abs((v - np.floor(v)) - 0.5) <= 1e-4
    print(f"share within 1e-4 of a half-integer: {band.mean():.5%}; mismatches outside: {(got != want)[~band].sum()}, inside: "
          f"{(got != want)[band].sum()}")
    assert band.mean() <= 1e-3
    assert np.array_equal(got[~band], want[~band])
    assert np.abs(got - want).max() <= 1
    # the ends and the model's own thresholds
    assert tm.encode(F([0.0, 1.0, -0.0]), tm.SRGB).tolist() == [0, 255, 0]
    T = tm.srgb_table()
    assert np.array_equal(tm.encode(T, tm.SRGB), np.arange(1, 256)) and np.array_equal(tm.encode(np.nextafter(T, F(0)), tm.SRGB), np.arange(255))


def test_linear_encode_truncates_like_the_display_packer():
    y = F([0.0, 1.0 / 255.0, np.nextafter(F(1.0), F(0.0)), 1.0, 0.5])
    assert tm.encode(y, tm.LINEAR).tolist() == [0, int(float(F(1.0 / 255.0)) * 255.0), 254, 255, 127]


# ---- 5: meter -------------------------------------------------------------------------------------------------------

def _grey_with_lum_bits(b):
    """A colour (0, g, 0) whose lum() has exactly the bit pattern b, or None."""
    want = tm.from_bits(np.uint32(b))
    g0 = F(want / F(0.7152))
    for g in (g0, np.nextafter(g0, F(0)), np.nextafter(g0, F(np.inf))):
        if tm.scalar_bits(tm.lum(np.array([0, g, 0], np.float32))) == b:
            return np.array([0, g, 0], np.float32)
    return None


def test_meter_known_answers():
    found = []
    for b in range(0x3E000000, 0x3E000000 + 400, 7):  # luminances near 0.125
        c = _grey_with_lum_bits(b)
        if c is not None:
            found.append((b, c))
    assert len(found) >= 2
    (A, ca), (B, cb) = found[0], found[-1]
    img = np.empty((4, 6, 3), np.float32)
    img[:2], img[2:] = ca, cb
    S, K = tm.meter(img)
    assert (S, K) == (12 * A + 12 * B, 24) and S // K == (A + B) // 2
    assert tm.scalar_bits(tm.target(S, K, 0.18, None)) == tm.scalar_bits(F(0.18) / tm.from_bits(np.uint32((A + B) // 2)))


def test_meter_excludes_what_it_should():
    rng = np.random.default_rng(1)
    img = np.exp2(rng.uniform(-10, 6, (9, 11, 3))).astype(np.float32)
    S, K = tm.meter(img)
    assert K == 99
    junk = np.zeros((8, 11, 3), np.float32)
    junk[0], junk[1], junk[2], junk[3] = np.nan, np.inf, -np.inf, -2.0
    junk[4], junk[5] = 0.0, 1e-42
    junk[6] = np.nextafter(F(2.0 ** -20), F(0))  # luminance just below 2^-20 (the weights sum to less than 1 ulp above 1)
    junk[7, :, 0], junk[7, :, 1] = np.inf, -np.inf  # inf - inf inside lum: NaN
    assert tm.meter(junk) == (0, 0)
    assert tm.meter(np.concatenate([img, junk])) == (S, K)
    # the ends of the range count
    assert tm.meter(_grey_with_lum_bits(tm.METER_MIN)[None, None])[1] == 1
    assert tm.meter(F([[[3.4e38, 3.4e38, 3.4e38]]]))[1] == 1  # (finite: the weights sum to 1)
    assert tm.meter(F([[[3.4e38, 3.4e38, np.inf]]]))[1] == 0
    # K = 0: the exposure is kept, 1 with no history
    assert tm.target(0, 0, 0.18, None) == F(1.0) and tm.target(0, 0, 0.18, F(0.37)) == F(0.37)
    outs, exps = tm.tonemap_sequence([img, junk, junk], rate=0.5)
    assert exps[1] == exps[0] and exps[2] == exps[0]
    outs, exps = tm.tonemap_sequence([junk, img])
    assert exps[0] == F(1.0) and exps[1] == tm.target(S, K, 0.18, None)


@pytest.mark.parametrize("seed", range(5))
def test_meter_is_a_geometric_mean_within_the_log2_gap(seed):
    img = tm.lognormal_image(400, 250, seed)
    S, K = tm.meter(img)
    assert K == 100_000
    lavg = float(tm.from_bits(np.uint32(S // K)))
    true = float(np.exp2(np.mean(np.log2(tm.lum(img).astype(np.float64)))))
    err = np.log2(lavg / true)
    print(f"seed {seed}: log2(Lavg / geometric mean) = {err:+.4f}")
    assert abs(err) <= tm.LOG2_GAP


def test_adapt_steps():
    assert tm.scalar_bits(tm.adapt(None, F(0.3), 0.5)) == tm.scalar_bits(F(0.3))
    assert tm.scalar_bits(tm.adapt(F(2.0), F(0.3), 1.0)) == tm.scalar_bits(F(0.3))
    assert tm.adapt(F(2.0), F(1.0), 0.25) == F(1.75)
    outs, exps = tm.tonemap_sequence(tm.stepped_frames(8, 8, 3), rate=0.5)
    assert all(exps[k + 1] < exps[k] for k in range(5))  # brighter frames: the exposure falls, half the way each time
    t = [tm.target(*tm.meter(f[..., :3]), 0.18, None) for f in tm.stepped_frames(8, 8, 3)]
    assert exps[0] == t[0] and exps[1] == t[0] + F(0.5) * (t[1] - t[0])


# ---- 6: curves ------------------------------------------------------------------------------------------------------

CLASSES = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1e-39, 1e-3, 0.18, 1.0, 4.0, 100.0, 65504.0, 1e30, 3.4e38], np.float32)


@pytest.mark.parametrize("curve", [tm.CLAMP, tm.REINHARD, tm.ACES])
@pytest.mark.parametrize("e", [1.0, 2.0 ** -20, 1e-38, 3e38])
def test_curves_stay_in_range_for_every_input_class(curve, e):
    grid = np.stack(np.meshgrid(CLASSES, CLASSES, CLASSES, indexing="ij"), axis=-1)
    y = tm.curve_map(grid, e, curve)
    assert y.dtype == np.float32 and not np.isnan(y).any() and (y >= 0).all() and (y <= 1).all()
    for enc in (tm.SRGB, tm.LINEAR):
        out = tm.map_encode(grid, e, curve, enc)
        assert out.dtype == np.uint8 and (out[..., 3] == 255).all()
    # a NaN, negative or -inf channel is black in CLAMP and ACES, whatever the others hold
    if curve != tm.REINHARD:
        assert (y[[0, 2, 3, 4]][..., 0] == 0).all() and (y[1][..., 0] == 1).all()  # (and +inf is white)


def test_reinhard_maps_white_to_one_exactly():
    """A grey whose luminance is `white` = 4: s = (1 + 4 / 16) / (1 + 4) = 0.25 exactly, y = 4 * 0.25 = 1 exactly, before the last clamp."""
    g = F(4.0)
    x = np.array([g, g, g], np.float32)
    lx = tm.lum(x)
    s = (F(1.0) + lx / (F(4.0) * F(4.0))) / (F(1.0) + lx)
    print(f"lum(4, 4, 4) = {float(lx)!r}, s = {float(s)!r}")
    assert x[0] * s == F(1.0)
    assert tm.bits(tm.curve_map(x, 1.0, tm.REINHARD))[0] == tm.scalar_bits(F(1.0))
    assert tm.map_encode(x, 1.0, tm.REINHARD).tolist() == [255, 255, 255, 255]
    below = tm.curve_map(np.array([3.5, 3.5, 3.5], np.float32), 1.0, tm.REINHARD)
    assert (below < 1).all() and (below > 0.9).all()
    # hue is kept: the channel ratios of y are those of x
    c = np.array([2.0, 1.0, 0.5], np.float32)
    y = tm.curve_map(c, 1.0, tm.REINHARD)
    assert y[0] / y[1] == 2.0 and y[1] / y[2] == 2.0


def test_aces_known_values():
    y = tm.curve_map(F([0.0, 0.18, 1.0]), 1.0, tm.ACES)
    assert y[0] == 0.0 and abs(float(y[1]) - 0.2669) < 1e-3 and abs(float(y[2]) - 0.8038) < 1e-3
    assert tm.curve_map(F([65504.0, 10.0, 0.5]), 1.0, tm.ACES)[0] == 1.0  # (the fit exceeds 1 above ~1.3 and is clamped)


def test_clamp_linear_at_exposure_one_is_the_display_packer(oracle):
    rng = np.random.default_rng(7)
    frame = rng.uniform(-0.3, 1.3, (23, 31, 14)).astype(np.float32)
    frame[0, :16, 0] = np.arange(16, dtype=np.float32) / F(255.0)
    frame[1, :16, 1] = np.nextafter(np.arange(16, dtype=np.float32) / F(255.0), F(0))
    frame[2, :4, 2] = [np.nan, np.inf, -np.inf, -0.0]
    want = oracle.display_pack(frame)[..., 2].copy().view(np.uint8).reshape(23, 31, 4)[..., :3]
    got = tm.map_encode(frame[..., :3], 1.0, tm.CLAMP, tm.LINEAR)
    assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all()


# ---- 7: the CLI -----------------------------------------------------------------------------------------------------

def _cli(tmp_path, args):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


CLI_REFUSALS = [
    (["--exposure", "2"], ["--exposure needs --tonemap"]),
    (["--tonemap-key", "0.2"], ["--tonemap-key needs --tonemap"]),
    (["--tonemap-white", "2"], ["--tonemap-white needs --tonemap"]),
    (["--tonemap-adapt", "0.5"], ["--tonemap-adapt needs --tonemap"]),
    (["--tonemap-encode", "srgb"], ["--tonemap-encode needs --tonemap"]),
    (["--tonemap", "filmic"], ["--tonemap 'filmic'", "clamp, reinhard or aces"]),
    (["--tonemap", "aces", "--batch", "--poses", "none.txt"], ["--tonemap cannot be combined with --batch"]),
    (["--tonemap", "aces", "--exposure", "0"], ["--exposure '0'", "auto or a finite number > 0"]),
    (["--tonemap", "aces", "--exposure", "bright"], ["--exposure 'bright'"]),
    (["--tonemap", "aces", "--exposure", "inf"], ["--exposure 'inf'"]),
    (["--tonemap", "aces", "--exposure", "-1"], ["--exposure '-1'"]),
    (["--tonemap", "aces", "--tonemap-key", "0"], ["--tonemap-key 0", "> 0"]),
    (["--tonemap", "aces", "--tonemap-key", "nan"], ["--tonemap-key", "> 0"]),
    (["--tonemap", "reinhard", "--tonemap-white", "0"], ["--tonemap-white 0"]),
    (["--tonemap", "reinhard", "--tonemap-white", "inf"], ["--tonemap-white"]),
    (["--tonemap", "aces", "--tonemap-adapt", "0"], ["--tonemap-adapt 0", "(0, 1]"]),
    (["--tonemap", "aces", "--tonemap-adapt", "1.5"], ["--tonemap-adapt 1.5", "(0, 1]"]),
    (["--tonemap", "aces", "--tonemap-encode", "rec709"], ["--tonemap-encode 'rec709'", "srgb or linear"]),
]


@pytest.mark.parametrize("args,words", CLI_REFUSALS, ids=[" ".join(a) for a, _ in CLI_REFUSALS])
def test_cli_refusals_come_before_any_device(tmp_path, args, words):
    """The device here would fail with a GPUassert line: none of these gets that far."""
    run = _cli(tmp_path, ["--size", "16", "--device", "99"] + args)
    assert run.returncode == 1, run.stderr
    assert run.stderr.startswith("ERROR: ") and "GPUassert" not in run.stderr, run.stderr
    for w in words:
        assert w in run.stderr, run.stderr


def test_cli_help_lists_the_flags(tmp_path):
    run = _cli(tmp_path, ["--help"])
    assert run.returncode == 0
    for opt in ("--tonemap arg", "--exposure", "--tonemap-key", "--tonemap-white", "--tonemap-adapt", "--tonemap-encode"):
        assert opt in run.stdout
