"""CPU tests of the denoiser's batch entry points (pt_denoiser_reserve_frames / _enqueue_frames / _denoise_frames and their
lab getters): exported, declared, covered by the ctypes tables, and refusing null arguments without a device."""
import ctypes
import os

import pytest

from conftest import ROOT

PT_EINVAL = -1
PRODUCT = ("pt_denoiser_reserve_frames", "pt_denoiser_enqueue_frames", "pt_denoiser_denoise_frames")
LAB = ("pt_debug_denoiser_last_enqueue", "pt_debug_denoiser_conv_plan")


def test_batch_symbols_are_exported_declared_and_in_the_tables(pt, lab):
    header = open(os.path.join(ROOT, "include", "ptcore.h")).read()
    lab_header = open(os.path.join(ROOT, "include", "ptcore_lab.h")).read()
    for name in PRODUCT:
        assert name + "(" in header and name in pt.ABI and hasattr(pt.lib, name), name
        assert hasattr(lab.lib, name), name
    for name in LAB:
        assert name + "(" in lab_header and name in lab.LAB_ABI and hasattr(lab.lib, name), name
        assert not hasattr(pt.lib, name), f"{name} is a lab diagnostic, not product ABI"
    assert pt.lib.pt_abi_version() == 6  # additive: the version stays


@pytest.mark.parametrize("call,word", [
    (lambda pt: pt.lib.pt_denoiser_reserve_frames(None, 8), "null denoiser"),
    (lambda pt: pt.lib.pt_denoiser_enqueue_frames(None, 2, None, 14, None, 0, None), "null denoiser"),
    (lambda pt: pt.lib.pt_denoiser_denoise_frames(None, 2, None, 14, None, 0, None), "null denoiser"),
], ids=["reserve", "enqueue", "denoise"])
def test_null_denoiser_is_refused_without_a_device(pt, call, word):
    assert call(pt) == PT_EINVAL
    msg = pt.lib.pt_last_error().decode()
    assert word in msg and "_frames" in msg, msg


def test_lab_getters_refuse_a_null_denoiser(lab):
    g, n = ctypes.c_int(7), ctypes.c_int(7)
    assert lab.lib.pt_debug_denoiser_last_enqueue(None, ctypes.byref(g), ctypes.byref(n)) == PT_EINVAL
    assert lab.lib.pt_debug_denoiser_conv_plan(None, 2, 0, (ctypes.c_int * 6)()) == PT_EINVAL
