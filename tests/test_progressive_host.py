"""CPU tests of progressive sessions' host side: the C ABI's argument checks, the Python view, and the CLI's --progressive
flag and its refusals (each before any device is touched: no GPUassert, no output file)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


def _pathtrace(args, tmp_path):
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    return subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)


def test_help_lists_progressive(tmp_path):
    run = _pathtrace(["--help"], tmp_path)
    assert run.returncode == 0 and "--progressive" in run.stdout


@pytest.mark.parametrize("extra, names", [
    (["--progressive", "2", "--frames", "3"], ["--progressive", "--frames"]),
    (["--progressive", "2", "--poses", "poses.txt"], ["--progressive", "--poses"]),
    (["--progressive", "2", "--poses", "poses.txt", "--batch"], ["--progressive", "--poses"]),
    (["--progressive", "2", "--batch"], ["--progressive", "--batch"]),
    (["--progressive", "2", "--gpus", "2"], ["--progressive", "--gpus"]),
    (["--progressive", "2", "--gpus", "1"], ["--progressive", "--gpus"]),
    (["--progressive", "0"], ["--progressive"]),
    (["--progressive", "-1"], ["--progressive"]),
    (["--progressive", "1", "-s", "1"], ["--progressive", "-s"]),
    (["--progressive", "3", "-s", "0"], ["--progressive", "-s"]),
    (["--progressive", "70000", "-s", "65536"], ["--progressive", "-s"]),
])
def test_cli_refusals(tmp_path, extra, names):
    (tmp_path / "poses.txt").write_text("50 52 295.6 -90 0\n")
    out = str(tmp_path / "o")
    run = _pathtrace(["--size", "16", "-o", out] + extra, tmp_path)
    assert run.returncode != 0
    assert "ERROR" in run.stderr and all(n in run.stderr for n in names), run.stderr
    assert "GPUassert" not in run.stderr
    assert not os.path.exists(out + ".exr")


def test_create_with_null_renderer_is_einval(pt):
    h = ctypes.c_void_p()
    assert pt.lib.pt_progressive_create(None, ctypes.byref(h)) == -1
    assert "NULL" in pt.lib.pt_last_error().decode()
    assert h.value is None
    assert pt.lib.pt_progressive_create(None, None) == -1


def test_null_session_arguments_are_einval(pt):
    n = ctypes.c_int64(0)
    v = ctypes.c_int(0)
    assert pt.lib.pt_progressive_samples(None, ctypes.byref(n)) == -1
    assert pt.lib.pt_progressive_variant(None, 9, ctypes.byref(v)) == -1
    assert pt.lib.pt_progressive_reset(None) == -1
    assert pt.lib.pt_progressive_enqueue(None, 4, None, None, 0, None, None, None) == -1
    assert pt.lib.pt_progressive_destroy(None) == 0


def test_python_view_exists(pt, lab):
    assert hasattr(pt, "Progressive")
    for m in ("enqueue", "render", "samples", "reset", "variant", "destroy"):
        assert callable(getattr(pt.Progressive, m))
    assert hasattr(lab.lib, "pt_debug_progressive_set_samples")
    assert not hasattr(pt.lib, "pt_debug_progressive_set_samples")
