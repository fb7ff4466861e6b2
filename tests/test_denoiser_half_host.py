"""CPU tests of the denoiser's half-precision mode (PT_DENOISE_F16, DENOISER.md "Half precision"): the rounding model and
the choice of fp16 over bf16 on the golden frames, the argument checks of pt_denoiser_create_opts (all before a device is
touched), no CPU fallback, the Python and CLI front ends, and the built product library's gfx950 assembly (an fp16 MFMA in
the half kernels, no scratch, no fp16 MFMA in the fp32 instances)."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_half_model as HM
from conftest import GOLDEN, ROOT

PT_EINVAL = -1
GOLDEN_FRAMES = ("oracle_64_spp4_xorwow", "oracle_64_spp1_xorwow", "oracle_64_spp4_philox")


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


@pytest.mark.parametrize("golden", GOLDEN_FRAMES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_error_is_display_sized_and_bf16_is_clearly_worse(dw, golden, seed, capsys):
    """The nine cases of the format decision: the fp16 model's error against the unrounded float64 network is at most 5e-3
    max and 8e-4 rms (1.5 x the worst seen: 3.1e-3, 5.2e-4), and rounding to bf16 at the same points has at least 2.5 x the
    fp16 rms (3.1 x was the smallest seen)."""
    frame = np.load(os.path.join(GOLDEN, golden + ".npz"))["image"].reshape(64, 64, 14).astype(np.float32)
    sdk = dw.random_state_dict(seed=seed)
    ref = HM.denoise(frame, sdk, None)
    mx, rms = HM.errors(HM.denoise(frame, sdk, "fp16"), ref)
    bmx, brms = HM.errors(HM.denoise(frame, sdk, "bf16"), ref)
    with capsys.disabled():
        print(f"\n{golden} seed {seed}: fp16 max {mx:.2e} rms {rms:.2e} | bf16 max {bmx:.2e} rms {brms:.2e} ({brms / rms:.1f}x)")
    assert mx <= 5e-3 and rms <= 8e-4
    assert brms >= 2.5 * rms


def test_model_without_rounding_is_the_restatement(dw):
    import denoise_restatement as R

    frame = np.load(os.path.join(GOLDEN, GOLDEN_FRAMES[0] + ".npz"))["image"].reshape(64, 64, 14).astype(np.float32)
    sdk = dw.random_state_dict(seed=1)
    assert np.array_equal(HM.denoise(frame, sdk, None), R.denoise(frame, sdk)[1])


def _create_opts(pt, blob, precision=1, max_frames=1, reserved=None, w=16, h=16):
    opts = pt.DenoiserOpts(precision=precision, max_frames=max_frames)
    for i, v in (reserved or {}).items():
        opts.reserved[i] = v
    handle = ctypes.c_void_p()
    rc = pt.lib.pt_denoiser_create_opts(w, h, blob, len(blob), ctypes.byref(opts), ctypes.byref(handle))
    return rc, pt.lib.pt_last_error().decode(), handle


def test_new_symbols_are_declared_exported_and_the_abi_version_stays(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    for name in ("pt_denoiser_create_opts", "pt_denoiser_create_opts_from_file", "pt_denoiser_precision"):
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name) and hasattr(lab.lib, name), name
    assert "PT_DENOISE_F32 = 0" in header and "PT_DENOISE_F16 = 1" in header
    assert ctypes.sizeof(pt.DenoiserOpts) == 32
    assert "pt_debug_denoiser_memory" in lab.LAB_ABI and not hasattr(pt.lib, "pt_debug_denoiser_memory")
    assert pt.lib.pt_abi_version() == 6


def test_create_opts_refuses_bad_options_before_a_device_is_touched(pt, dw, sd):
    blob = dw.to_bytes(sd)
    rc, msg, _ = _create_opts(pt, blob, precision=2)
    assert rc == PT_EINVAL and "precision 2" in msg
    rc, msg, _ = _create_opts(pt, blob, precision=-1)
    assert rc == PT_EINVAL and "precision" in msg
    rc, msg, _ = _create_opts(pt, blob, reserved={3: 7})
    assert rc == PT_EINVAL and "reserved[3]" in msg
    for mf in (0, -4):
        rc, msg, _ = _create_opts(pt, blob, max_frames=mf)
        assert rc == PT_EINVAL and "max_frames" in msg
    rc, msg, _ = _create_opts(pt, blob, max_frames=70000)
    assert rc == PT_EINVAL and "max_frames" in msg
    handle = ctypes.c_void_p()
    assert pt.lib.pt_denoiser_create_opts(16, 16, blob, len(blob), None, ctypes.byref(handle)) == PT_EINVAL
    assert "null options" in pt.lib.pt_last_error().decode()
    v = ctypes.c_int(5)
    assert pt.lib.pt_denoiser_precision(None, ctypes.byref(v)) == PT_EINVAL and "null denoiser" in pt.lib.pt_last_error().decode()


def test_half_create_refuses_a_weight_outside_the_fp16_range_by_name(pt, dw, sd):
    big = dict(sd)
    big["block2.conv1.weight"] = sd["block2.conv1.weight"].copy()
    big["block2.conv1.weight"][3, 2, 1, 0] = 1e5
    blob = dw.to_bytes(big)
    rc, msg, _ = _create_opts(pt, blob, precision=1)
    assert rc == PT_EINVAL and "block2.conv1.weight" in msg and "65504" in msg, msg
    neg = dict(sd)
    neg["rgb_conv.weight"] = sd["rgb_conv.weight"].copy()
    neg["rgb_conv.weight"][0, 0, 0, 0] = -65600.0
    rc, msg, _ = _create_opts(pt, dw.to_bytes(neg), precision=1)
    assert rc == PT_EINVAL and "rgb_conv.weight" in msg
    # batch-norm parameters and biases stay fp32 in the half mode: they are not range-checked (and fp32 mode never is)
    bn = dict(sd)
    bn["block1.bn1.running_var"] = sd["block1.bn1.running_var"] * np.float32(1e6)
    if not _have_gpu(pt):
        rc, msg, _ = _create_opts(pt, dw.to_bytes(bn), precision=1)
        assert rc in (-2, -3), msg
        rc, msg, _ = _create_opts(pt, blob, precision=0)
        assert rc in (-2, -3), msg
    with pytest.raises(pt.PtError) as e:
        pt.Denoiser(16, 16, big, precision="half")
    assert e.value.code == PT_EINVAL and "block2.conv1.weight" in str(e.value)


def test_valid_half_create_fails_loudly_without_a_gpu(pt, dw, sd):
    """No CPU fallback in the half mode either: PT_ENODEVICE / PT_EHIP naming the device."""
    if _have_gpu(pt):
        return  # tests/test_denoiser_half_gpu.py creates half denoisers there
    with pytest.raises(pt.PtError) as e:
        pt.Denoiser(16, 16, sd, precision="half")
    assert e.value.code in (-2, -3) and "device" in str(e.value).lower()
    with pytest.raises(pt.PtError) as e:
        pt.denoise_frame(np.zeros((16, 16, 14), np.float32), sd, precision="half")
    assert e.value.code in (-2, -3)


def test_python_precision_argument(pt, sd):
    assert pt.denoise_precision("float32") == pt.DENOISE_F32 == 0 and pt.denoise_precision("half") == pt.DENOISE_F16 == 1
    for bad in ("fp16", "bf16", "float16", 1, None):
        with pytest.raises(ValueError):
            pt.Denoiser(16, 16, sd, precision=bad)
    with pytest.raises(pt.PtError) as e:
        pt.Denoiser(16, 16, sd, max_frames=0, precision="half")
    assert e.value.code == PT_EINVAL and "max_frames" in str(e.value)


def _pathtrace(args, tmp_path):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


def test_cli_refuses_a_bad_denoise_precision_before_a_device_is_touched(pt, dw, sd, tmp_path):
    good = str(tmp_path / "good.ptdn")
    dw.export(sd, good)
    out = str(tmp_path / "o")
    run = _pathtrace(["--size", "16", "--denoise-precision", "half", "-o", out, "--nobitmap"], tmp_path)
    assert run.returncode != 0 and "--denoise-precision needs -d" in run.stderr
    for bad in ("bf16", "fp16", "double", ""):
        run = _pathtrace(["--size", "16", "-d", "--denoise-weights", good, "--denoise-precision", bad, "-o", out, "--nobitmap"], tmp_path)
        assert run.returncode != 0 and ("half or float" in run.stderr or "--denoise-precision" in run.stderr), run.stderr
    run = _pathtrace(["--size", "16", "-d", "--denoise-weights", good, "--denoise-precision"], tmp_path)
    assert run.returncode != 0 and "--denoise-precision" in run.stderr
    assert not os.path.exists(out + ".exr")
    assert "--denoise-precision" in _pathtrace(["--help"], tmp_path).stdout


def _functions(asm):
    """{mangled name: body text} of every function of a gfx950 assembly file."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        out[m.group(1)] = m.group(0)
    return out


def test_product_assembly_has_fp16_mfma_only_in_the_half_kernels_and_no_scratch(pt):
    paths = glob.glob(os.path.join(ROOT, "cuda-pathtrace_amd", "csrc", "build", "prod", "pt_denoise*-gfx950.s"))
    assert len(paths) == 1, paths
    asm = open(paths[0]).read()
    fns = _functions(asm)
    # one kernel family templated on the stored element: the Itanium mangling of the first template argument is DF16_ for
    # _Float16 and f for float
    half = {n: b for n, b in fns.items() if "ptdn11conv_kernelIDF16_" in n}
    fp32 = {n: b for n, b in fns.items() if "ptdn11conv_kernelIfL" in n}
    assert len(half) == 5 and len(fp32) == 5, sorted(fns)
    for n, b in half.items():
        assert "v_mfma_f32_32x32x16_f16" in b and "v_mfma_f32_32x32x2_f32" not in b, n
        assert "ds_read_b128" in b or "ds_load_b128" in b, n  # B fragments: one 16-byte LDS read each
    for n, b in fp32.items():
        assert "v_mfma_f32_32x32x2_f32" in b and "_f16" not in b.replace(n, ""), n
    # the saturating store: clamp in fp32 (v_med3_f32), then convert
    for key in ("splitk_reduce_kernelIDF16_", "pre_apply_kernelIDF16_"):
        (body,) = [b for n, b in fns.items() if key in n]
        assert "v_med3_f32" in body and ("v_cvt_f16_f32" in body or "v_cvt_pk_f16_f32" in body), key
    # the mirror image: no float instance picked up the half store or a half load
    (reduce32,) = [b for n, b in fns.items() if "splitk_reduce_kernelIfE" in n]
    (pre32,) = [b for n, b in fns.items() if "pre_apply_kernelIfE" in n]
    for b in list(fp32.values()) + [reduce32, pre32]:
        name = b.split(":", 1)[0]
        code = b.replace(name, "")
        assert not re.search(r"v_cvt\w*_f16", code) and "v_cvt_f32_f16" not in code and "v_med3_f32" not in code, name
    # no scratch in any kernel of the file: the metadata of every half kernel says 0 bytes
    meta = re.findall(r"\.name:\s+(_ZN4ptdn\w+)\n\s+\.private_segment_fixed_size:\s+(\d+)", asm)
    names = [n for n, _ in meta]
    for key in ("conv_kernelIDF16_", "splitk_reduce_kernelIDF16_", "pre_apply_kernelIDF16_"):
        assert any(key in n for n in names), key
    assert all(int(sz) == 0 for _, sz in meta), meta
    for n, b in half.items():
        assert "scratch_" not in b and "buffer_store_dword" not in b, n
