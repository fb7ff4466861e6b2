"""CPU tests of the denoiser's host side: the PTDN weight format (cuda-pathtrace_amd/denoise_weights.py writes it, the
library's loader checks it), the loader's refusals (each names the offending key), no CPU fallback, and the CLI's -d."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


@pytest.fixture(scope="module")
def sd(dw):
    return dw.random_state_dict(seed=3)


def _have_gpu(pt):
    try:
        return pt.device_count() > 0
    except pt.PtError:
        return False


def _rejects(pt, blob, *words):
    with pytest.raises(pt.PtError) as e:
        pt.denoiser_weights_check(blob)
    assert e.value.code == -1
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_expected_shapes_are_the_reference_network(dw):
    shapes = dw.expected_shapes()
    assert len(shapes) == 136
    n = sum(int(np.prod(s)) for s in shapes.values())
    assert 25.2e6 < n < 25.4e6  # 25.3 M fp32 parameters (101 MB)
    assert shapes["block6.conv2.weight"] == (1024, 1024, 3, 3) and shapes["block1.res_conv.weight"] == (32, 14, 3, 3)
    assert shapes["lat_0.weight"] == (32, 14, 1, 1) and shapes["backwards_10.weight"] == (32, 32, 3, 3)
    assert shapes["rgb_conv.weight"] == (3, 32, 3, 3)


def test_random_state_dict_is_seeded_with_non_trivial_batch_norm(dw, sd):
    again = dw.random_state_dict(seed=3)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert not np.array_equal(sd["block2.conv1.weight"], dw.random_state_dict(seed=4)["block2.conv1.weight"])
    for k, v in sd.items():
        assert v.dtype == np.float32 and v.shape == dw.expected_shapes()[k]
        if "bn" in k and not k.endswith("running_mean"):
            assert np.all(v != 1.0) and 0.5 < float(np.mean(v)) < 1.5, k
        if k.endswith("running_mean"):
            assert np.all(v != 0.0) and abs(float(np.mean(v))) < 0.05, k
    w = sd["block4.conv2.weight"]
    assert abs(float(w.std()) - np.sqrt(2.0 / (256 * 9))) < 2e-3  # He scaling
    iw = dw.random_state_dict(seed=3, integer=True)["block1.conv1.weight"]
    assert np.array_equal(iw, np.round(iw)) and iw.min() == -3 and iw.max() == 3 and iw.mean() > 0  # asymmetric


def test_export_and_validator_round_trip(pt, dw, sd, tmp_path):
    path = str(tmp_path / "w.ptdn")
    dw.export(sd, path)
    blob = open(path, "rb").read()
    assert blob[:4] == b"PTDN" and struct.unpack_from("<II", blob, 4) == (1, 136)
    pt.denoiser_weights_check(path)
    pt.denoiser_weights_check(blob)
    pt.denoiser_weights_check(sd)
    back = dw.from_bytes(blob)
    assert list(back) == list(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    # torch tensors and num_batches_tracked entries (a real train.py state_dict) are accepted; the counters are dropped
    import torch

    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    tsd["block1.bn1.num_batches_tracked"] = torch.tensor(7)
    assert dw.to_bytes(tsd) == blob


def test_validator_rejects_missing_extra_and_wrong_shape(pt, dw, sd):
    missing = dict(sd)
    del missing["block3.bn1.running_var"]
    _rejects(pt, dw.to_bytes(missing), "missing", "block3.bn1.running_var")
    extra = dict(sd)
    extra["block7.conv1.weight"] = np.zeros((2, 2), np.float32)
    _rejects(pt, dw.to_bytes(extra), "unexpected", "block7.conv1.weight")
    wrong = dict(sd)
    wrong["lat_2.weight"] = np.zeros((32, 64, 3, 3), np.float32)
    _rejects(pt, dw.to_bytes(wrong), "lat_2.weight", "(32, 64, 3, 3)", "(32, 64, 1, 1)")
    flat = dict(sd)
    flat["rgb_conv.bias"] = np.zeros((1, 3), np.float32)
    _rejects(pt, dw.to_bytes(flat), "rgb_conv.bias")


def test_validator_rejects_truncation_trailing_bytes_and_bad_headers(pt, dw, sd):
    blob = dw.to_bytes(sd)
    _rejects(pt, blob[:-4], "truncated", "rgb_conv.bias")
    _rejects(pt, blob[:len(blob) // 2], "truncated")
    _rejects(pt, blob[:6], "PTDN")
    _rejects(pt, blob + b"\0\0\0\0", "trailing")
    _rejects(pt, b"NDTP" + blob[4:], "magic")
    _rejects(pt, blob[:4] + struct.pack("<I", 2) + blob[8:], "version")
    twice = dw.to_bytes(sd) + dw.to_bytes({"lat_0.bias": sd["lat_0.bias"]})[12:]
    twice = twice[:8] + struct.pack("<I", 137) + twice[12:]
    _rejects(pt, twice, "lat_0.bias", "twice")


def test_create_validates_before_anything_else_and_fails_loudly_without_gpu(pt, dw, sd, tmp_path):
    """No CPU fallback: a valid file on a machine without a device gives PT_ENODEVICE / PT_EHIP; bad arguments and bad files
    are refused first, with PT_EINVAL."""
    for w, h in ((0, 16), (16, -1), (5000, 5000)):
        with pytest.raises(pt.PtError) as e:
            pt.Denoiser(w, h, sd)
        assert e.value.code == -1
    bad = dict(sd)
    del bad["lat_0.weight"]
    with pytest.raises(pt.PtError) as e:
        pt.Denoiser(16, 16, bad)
    assert e.value.code == -1 and "lat_0.weight" in str(e.value)
    import ctypes

    h = ctypes.c_void_p()
    rc = pt.lib.pt_denoiser_create_from_file(16, 16, str(tmp_path / "nope.ptdn").encode(), ctypes.byref(h))
    assert rc == -1 and b"cannot open" in pt.lib.pt_last_error()
    if _have_gpu(pt):
        pytest.skip("a GPU is present (tests/test_denoiser_gpu.py covers creation there)")
    with pytest.raises(pt.PtError) as e:
        pt.Denoiser(16, 16, sd)
    assert e.value.code in (-2, -3) and "device" in str(e.value).lower()


def _pathtrace(args, tmp_path):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


def test_cli_denoising_needs_valid_weights(pt, dw, sd, tmp_path):
    out = str(tmp_path / "o")
    run = _pathtrace(["--size", "16", "-d", "-o", out, "--nobitmap"], tmp_path)
    assert run.returncode != 0 and "--denoise-weights" in run.stderr
    bad = dict(sd)
    bad["lat_3.bias"] = np.zeros(31, np.float32)
    path = str(tmp_path / "bad.ptdn")
    dw.export(bad, path)
    run = _pathtrace(["--size", "16", "-d", "--denoise-weights", path, "-o", out, "--nobitmap"], tmp_path)
    assert run.returncode != 0 and "lat_3.bias" in run.stderr
    good = str(tmp_path / "good.ptdn")
    dw.export(sd, good)
    run = _pathtrace(["--size", "16", "-d", "--denoise-weights", good, "--poses", good, "--batch", "-o", out], tmp_path)
    assert run.returncode != 0 and "--batch" in run.stderr
    run = _pathtrace(["--size", "16", "-i", "-o", out], tmp_path)
    assert run.returncode != 0 and "-i" in run.stderr
    assert not os.path.exists(out + ".exr")
