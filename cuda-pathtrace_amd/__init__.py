"""cuda-pathtrace_amd -- MI355X (gfx950) implementation of cuda-pathtrace's per-pixel
Monte-Carlo megakernel, behind the C ABI of include/ptcore.h.

This Python module is only the ctypes view of libptcore.so used by tests/, bench.py and the
multi-GPU driver (one process per GPU under torch.distributed).  The product is the shared
library and the C++ look-alike headers in host/; nothing here computes pixels, and there is
no CPU fallback: importing works without a GPU (the library loads), every compute call
raises PtError when no HIP device is usable, and a missing libptcore.so raises at import.

The directory name has a hyphen (it is fixed by the project layout), so import it through
`load_package()` in __graft_entry__.py / tests/conftest.py, which registers it as
`cuda_pathtrace_amd`.
"""
import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PT_LIB_OVERRIDE: another build of the same library -- A/B experiments (tools/ab_tiles.py) and the lab build
# libptcore_lab.so (experimental kernel variants + pt_debug_* diagnostics; __graft_entry__.load_lab())
LIB_PATH = os.environ.get("PT_LIB_OVERRIDE") or os.path.join(_HERE, "libptcore.so")
LAB_LIB_PATH = os.path.join(_HERE, "libptcore_lab.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C cuda-pathtrace_amd/csrc` "
        "(or __graft_entry__.build()); there is no fallback implementation"
    )

RNG_XORWOW = 0
RNG_PHILOX = 1
CHANNELS = 14

SPHERE_DTYPE = np.dtype([("radius", "<f4"), ("pos", "<f4", 3), ("emission", "<f4", 3), ("color", "<f4", 3)])
assert SPHERE_DTYPE.itemsize == 40


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptcore error {code}: {msg}")
        self.code = code


class RendererOpts(ctypes.Structure):
    _fields_ = [
        ("max_bounces", ctypes.c_int32),
        ("rng_mode", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("row_begin", ctypes.c_int32),
        ("row_end", ctypes.c_int32),
        ("persist_rng", ctypes.c_int32),
        ("variant", ctypes.c_int32),
        ("layout", ctypes.c_int32),
        ("fast_math", ctypes.c_int32),
        ("chunks", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


VARIANT_FAST = 100
VARIANT_MATERIALS = 101  # PT_VARIANT_MATERIALS: what kernel_info reports while a material table is set
VARIANT_MATERIALS_LIGHTS = 102  # PT_VARIANT_MATERIALS_LIGHTS: ... while direct light sampling is on (Renderer.set_light_sampling)
VARIANT_MATERIALS_SKY = 103  # PT_VARIANT_MATERIALS_SKY: ... while a sky is set (Renderer.set_sky)
VARIANT_MATERIALS_LIGHTS_SKY = 104  # PT_VARIANT_MATERIALS_LIGHTS_SKY: ... a sky and direct light sampling
LAYOUT_INTERLEAVED, LAYOUT_PLANAR = 0, 1
# sphere materials (pt_material, include/ptcore.h; EXACTNESS.md A.22)
MATERIAL_DIFFUSE, MATERIAL_MIRROR, MATERIAL_GLOSSY, MATERIAL_GLASS = 0, 1, 2, 3
MATERIAL_DTYPE = np.dtype([("kind", "<i4"), ("param", "<f4")])
MATERIALS_MAX_SPHERES = 64
# smallpt's Cornell box: sphere 6 a mirror ball, sphere 7 a glass ball, everything else diffuse
SMALLPT_MATERIALS = [(MATERIAL_DIFFUSE, 0.0)] * 6 + [(MATERIAL_MIRROR, 0.0), (MATERIAL_GLASS, 1.5), (MATERIAL_DIFFUSE, 0.0)]
GATHER_AUTO, GATHER_RCCL, GATHER_PEER_COPY = 0, 1, 2


class AdaptiveOpts(ctypes.Structure):  # pt_adaptive_opts
    _fields_ = [
        ("tolerance", ctypes.c_float),
        ("floor", ctypes.c_float),
        ("min_samples", ctypes.c_int32),
        ("radius", ctypes.c_int32),
    ]


REC_WORDS = 26  # PT_CHUNK_WORDS (csrc/pt_kernel.h): words per tile pixel of a session's record

# Progressive.set_adaptive's defaults (profiles/adaptive/README.md: how they were chosen)
ADAPTIVE_FLOOR, ADAPTIVE_MIN_SAMPLES, ADAPTIVE_RADIUS = 0.05, 16, 1


class MgpuOpts(ctypes.Structure):
    _fields_ = [
        ("gather", ctypes.c_int32),
        ("force_exchange", ctypes.c_int32),
        ("timeout_ms", ctypes.c_int32),
        ("bands", ctypes.c_int32),
    ]


class KernelInfo(ctypes.Structure):
    _fields_ = [
        ("block_threads", ctypes.c_int32),
        ("grid_blocks", ctypes.c_int32),
        ("lds_bytes", ctypes.c_int32),
        ("num_vgprs", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("scratch_bytes", ctypes.c_int32),
        ("max_spheres", ctypes.c_int32),
        ("variant", ctypes.c_int32),
    ]


_fp = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); this table is also what tests check against include/ptcore.h
ABI = {
    "pt_abi_version": (ctypes.c_int, []),
    "pt_build_fingerprint": (ctypes.c_char_p, []),
    "pt_last_error": (ctypes.c_char_p, []),
    "pt_set_device": (ctypes.c_int, [ctypes.c_int]),
    "pt_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "pt_device_info": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pt_malloc": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_size_t]),
    "pt_free": (ctypes.c_int, [_vp]),
    "pt_memcpy_h2d": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    "pt_memcpy_d2h": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    "pt_memset": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_size_t]),
    "pt_device_synchronize": (ctypes.c_int, []),
    "pt_renderer_opts_default": (None, [ctypes.POINTER(RendererOpts)]),
    "pt_renderer_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RendererOpts), ctypes.POINTER(_vp)]),
    "pt_renderer_destroy": (ctypes.c_int, [_vp]),
    "pt_renderer_render": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _fp, _fp, _fp]),
    "pt_renderer_enqueue": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _fp, _fp, _vp]),
    "pt_renderer_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_int, _fp, _fp, _vp]),
    "pt_renderer_check": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]),
    "pt_renderer_set_display": (ctypes.c_int, [_vp, _vp]),
    "pt_renderer_set_frame": (ctypes.c_int, [_vp, ctypes.c_uint32]),
    "pt_renderer_reset_rng": (ctypes.c_int, [_vp]),
    "pt_renderer_get_rng_state": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    "pt_renderer_set_rng_state": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    "pt_renderer_kernel_info": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(KernelInfo)]),
    "pt_material_check": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_renderer_set_materials": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "pt_renderer_set_light_sampling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_sky_check": (ctypes.c_int, [_vp]),
    "pt_renderer_set_sky": (ctypes.c_int, [_vp, _vp]),
    "pt_mgpu_opts_default": (None, [ctypes.POINTER(MgpuOpts)]),
    "pt_mgpu_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(RendererOpts), ctypes.POINTER(MgpuOpts), ctypes.POINTER(_vp)]),
    "pt_mgpu_destroy": (ctypes.c_int, [_vp]),
    "pt_mgpu_render": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _fp, _fp, _fp]),
    "pt_mgpu_tile": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int), _fp]),
    "pt_mgpu_backend": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "pt_mgpu_frame_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), _fp, _fp]),
    "pt_scene_cornell": (ctypes.c_int, [_vp]),
    "pt_scene_random": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, _vp]),
    "pt_camera_basis": (ctypes.c_int, [_fp, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, _fp]),
    "pt_camera_basis_up": (ctypes.c_int, [_fp, ctypes.c_float, ctypes.c_float, _fp, ctypes.c_int, ctypes.c_int, _fp]),
    "pt_display_pack": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "pt_denoiser_weights_check": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "pt_denoiser_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "pt_denoiser_create_from_file": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_vp)]),
    "pt_denoiser_destroy": (ctypes.c_int, [_vp]),
    "pt_denoiser_create_opts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, _vp, ctypes.POINTER(_vp)]),
    "pt_denoiser_create_opts_from_file": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, _vp, ctypes.POINTER(_vp)]),
    "pt_denoiser_precision": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "pt_denoiser_enqueue": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "pt_denoiser_denoise": (ctypes.c_int, [_vp, _vp, _vp, _fp]),
    "pt_denoiser_reserve_frames": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_denoiser_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pt_denoiser_denoise_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _fp]),
    "pt_filter_opts_default": (None, [_vp]),
    "pt_filter_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "pt_filter_destroy": (ctypes.c_int, [_vp]),
    "pt_filter_reserve_frames": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_filter_workspace_bytes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_filter_spatial_opts_default": (None, [_vp]),
    "pt_filter_spatial_check": (ctypes.c_int, [_vp]),
    "pt_filter_set_spatial": (ctypes.c_int, [_vp, _vp]),
    "pt_filter_enqueue": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "pt_filter_run": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _fp]),
    "pt_filter_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "pt_filter_run_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _fp]),
    "pt_temporal_opts_default": (None, [_vp]),
    "pt_temporal_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "pt_temporal_destroy": (ctypes.c_int, [_vp]),
    "pt_temporal_reset": (ctypes.c_int, [_vp]),
    "pt_temporal_workspace_bytes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_temporal_camera": (ctypes.c_int, [_fp, _fp]),
    "pt_temporal_antilag_opts_default": (None, [_vp]),
    "pt_temporal_antilag_check": (ctypes.c_int, [_vp, ctypes.c_float]),
    "pt_temporal_set_antilag": (ctypes.c_int, [_vp, _vp]),
    "pt_temporal_fast": (ctypes.c_int, [_vp, _vp, _vp]),
    "pt_temporal_enqueue": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, _vp]),
    "pt_temporal_run": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, _fp]),
    "pt_temporal_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _fp, _fp, ctypes.c_int, _vp, _vp]),
    "pt_temporal_run_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _fp, _fp, ctypes.c_int, _vp, _fp]),
    "pt_temporal_scene_check": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp]),
    "pt_temporal_motion": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _fp, _fp, _vp, _vp]),
    "pt_temporal_enqueue_motion": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, _vp, _vp]),
    "pt_temporal_run_motion": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, _vp, _fp]),
    "pt_temporal_enqueue_scene": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, ctypes.c_int, _vp, _vp]),
    "pt_temporal_run_scene": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _fp, _fp, _vp, ctypes.c_int, _vp, _fp]),
    "pt_temporal_enqueue_frames_scenes": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _fp, _fp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "pt_temporal_run_frames_scenes": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _fp, _fp, _vp, ctypes.c_int, ctypes.c_int, _vp, _fp]),
    "pt_tonemap_opts_default": (None, [_vp]),
    "pt_tonemap_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "pt_tonemap_destroy": (ctypes.c_int, [_vp]),
    "pt_tonemap_reset": (ctypes.c_int, [_vp]),
    "pt_tonemap_workspace_bytes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_tonemap_reserve_frames": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_tonemap_srgb_table": (ctypes.c_int, [_fp]),
    "pt_tonemap_enqueue": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp]),
    "pt_tonemap_run": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _fp]),
    "pt_tonemap_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, _vp]),
    "pt_tonemap_run_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, _fp]),
    "pt_tonemap_exposure": (ctypes.c_int, [_vp, _fp]),
    "pt_compare_opts_default": (None, [_vp]),
    "pt_compare_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "pt_compare_destroy": (ctypes.c_int, [_vp]),
    "pt_compare_workspace_bytes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_compare_reserve_frames": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_compare_ssim_weights": (ctypes.c_int, [_fp]),
    "pt_compare_enqueue": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp]),
    "pt_compare_run": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _fp]),
    "pt_compare_enqueue_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp,
                                                 ctypes.c_size_t, _vp]),
    "pt_compare_run_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp,
                                             ctypes.c_size_t, _fp]),
    "pt_compare_result": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "pt_patches_opts_default": (None, [_vp]),
    "pt_patches_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "pt_patches_destroy": (ctypes.c_int, [_vp]),
    "pt_patches_workspace_bytes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_patches_prepare": (ctypes.c_int, [_vp, _vp, _vp]),
    "pt_patches_score": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp]),
    "pt_patches_result": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "pt_patches_gather": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "pt_patches_run_prepare": (ctypes.c_int, [_vp, _vp, _fp]),
    "pt_patches_run_score": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _fp]),
    "pt_patches_run_gather": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _fp]),
    "pt_progressive_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "pt_progressive_reset": (ctypes.c_int, [_vp]),
    "pt_progressive_enqueue": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _fp, _fp, _vp]),
    "pt_progressive_render": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _fp, _fp, _fp]),
    "pt_progressive_samples": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "pt_progressive_variant": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "pt_progressive_destroy": (ctypes.c_int, [_vp]),
    "pt_progressive_set_adaptive": (ctypes.c_int, [_vp, _vp]),
    "pt_progressive_active": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "pt_progressive_counts": (ctypes.c_int, [_vp, _vp, _vp]),
}
# include/ptcore_lab.h: only libptcore_lab.so exports these
LAB_ABI = {
    "pt_debug_unary_map": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t]),
    "pt_debug_unary_compare": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_div_compare": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_grid_header": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_grid_image": (ctypes.c_int, [_vp, ctypes.c_int, _fp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "pt_debug_primary_masks": (ctypes.c_int, [_vp, ctypes.c_int, _fp, _fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "pt_debug_primary_lists": (ctypes.c_int, [_vp, ctypes.c_int, _fp, _fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_policy_ms": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "pt_debug_policy_choice": (ctypes.c_int, [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "pt_debug_renderer_batch_launches": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_kernel_builds": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32)]),
    "pt_debug_variant_row": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32)]),
    "pt_debug_launch_census": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "pt_debug_launch_census_reset": (ctypes.c_int, []),
    "pt_debug_fast_nearest": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _vp, _vp]),
    "pt_debug_denoiser_layer_info": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                    ctypes.c_char_p, ctypes.c_size_t]),
    "pt_debug_denoiser_activation": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t]),
    "pt_debug_denoiser_set_activation": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t]),
    "pt_debug_denoiser_conv_info": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                   ctypes.c_char_p, ctypes.c_size_t]),
    "pt_debug_denoiser_run_conv": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "pt_debug_denoiser_activation_frames": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_size_t]),
    "pt_debug_denoiser_set_activation_frames": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_size_t]),
    "pt_debug_denoiser_run_conv_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t]),
    "pt_debug_denoiser_run_pre": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_int]),
    "pt_debug_denoiser_memory": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "pt_debug_denoiser_last_enqueue": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pt_debug_denoiser_conv_plan": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "pt_debug_filter_step": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int]),
    "pt_debug_filter_tiled": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pt_debug_filter_state": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, _vp, _vp, _vp]),
    "pt_debug_progressive_set_samples": (ctypes.c_int, [_vp, ctypes.c_int64]),
    "pt_debug_progressive_record": (ctypes.c_int, [_vp, _vp]),
    "pt_debug_progressive_set_active": (ctypes.c_int, [_vp, _vp]),
    "pt_debug_adaptive_select": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(AdaptiveOpts), _vp, _vp, _vp, _vp, _vp]),
    "pt_debug_adaptive_finalize": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_int, _vp]),
}

FN_INV_SQRT_LITERAL, FN_INV_SQRT_FAST, FN_SQRT_LITERAL, FN_SQRT_FAST, FN_SIN, FN_COS, FN_UNIFORM = range(7)
FN_ONEMINUS_LITERAL, FN_ONEMINUS_FAST, FN_ONEMINUS_F32, FN_ONEMINUS_F32_FLAG, FN_ZERO = 7, 8, 9, 10, 11
FN_UNIFORM_LITERAL = 12
FN_SIN_LITERAL, FN_COS_LITERAL = 13, 14

lib = ctypes.CDLL(LIB_PATH)
for _name, (_res, _args) in ABI.items():
    if os.environ.get("PT_LIB_OVERRIDE") and not hasattr(lib, _name):
        continue  # A/B tooling only: an alternative build of an older ABI (tools/build_alt.sh from an older tree)
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export the ABI
    _fn.restype = _res
    _fn.argtypes = _args
IS_LAB = hasattr(lib, "pt_debug_unary_map")
if IS_LAB:
    for _name, (_res, _args) in LAB_ABI.items():
        _fn = getattr(lib, _name)
        _fn.restype = _res
        _fn.argtypes = _args


def variants():
    """Kernel variants compiled into the loaded library (product: 0, 6, 8, 9, 10, 13, 14; lab adds 1-5, 7, 11, 12)."""
    out = []
    o = RendererOpts()
    for v in range(15):
        lib.pt_renderer_opts_default(ctypes.byref(o))
        o.variant = v
        h = _vp()
        rc = lib.pt_renderer_create(8, 8, 1, 8, ctypes.byref(o), ctypes.byref(h))
        if rc == 0:
            lib.pt_renderer_destroy(h)
            out.append(v)
        elif rc != -1:  # anything but "not in this build" is a real failure (no device ...)
            check(rc)
    return out


def build_fingerprint():
    return lib.pt_build_fingerprint().decode()


def check(rc):
    if rc != 0:
        raise PtError(rc, lib.pt_last_error().decode("utf-8", "replace"))


def _f32(a, n):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(n)
    return a, a.ctypes.data_as(_fp)


# ---- host-side inputs -----------------------------------------------------------------
def scene_cornell():
    s = np.zeros(9, dtype=SPHERE_DTYPE)
    check(lib.pt_scene_cornell(s.ctypes.data))
    return s


def scene_random(n, seed=0, with_walls=True):
    s = np.zeros(n, dtype=SPHERE_DTYPE)
    check(lib.pt_scene_random(n, seed, 1 if with_walls else 0, s.ctypes.data))
    return s


DEFAULT_EYE = (50.0, 52.0, 295.6)  # src/main.cu:24


def camera_basis(pos=DEFAULT_EYE, yaw=-90.0, pitch=0.0, width=512, height=512, world_up=None):
    p, pp = _f32(pos, 3)
    out = np.zeros(12, dtype=np.float32)
    if world_up is None:
        check(lib.pt_camera_basis(pp, yaw, pitch, width, height, out.ctypes.data_as(_fp)))
    else:
        u, up = _f32(world_up, 3)
        check(lib.pt_camera_basis_up(pp, yaw, pitch, up, width, height, out.ctypes.data_as(_fp)))
    return out


# ---- device ---------------------------------------------------------------------------
def device_count():
    n = ctypes.c_int(0)
    check(lib.pt_device_count(ctypes.byref(n)))
    return n.value


def set_device(i):
    check(lib.pt_set_device(i))


def device_info():
    name = ctypes.create_string_buffer(256)
    cus = ctypes.c_int(0)
    khz = ctypes.c_int(0)
    check(lib.pt_device_info(name, 256, ctypes.byref(cus), ctypes.byref(khz)))
    return {"name": name.value.decode(), "compute_units": cus.value, "clock_khz": khz.value}


def display_pack(frame):
    """pt_display_pack on a host [rows][cols][14] frame (uploads, packs on the GPU, downloads)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[0], frame.shape[1]
    din, dout = DeviceBuffer(frame.nbytes).upload(frame), DeviceBuffer(h * w * 12)
    try:
        check(lib.pt_display_pack(din.ptr, w, h, dout.ptr, None))
        check(lib.pt_device_synchronize())
        return dout.download(np.float32, (h, w, 3))
    finally:
        din.free()
        dout.free()


def unary_map(fn, x):
    """Evaluate device building block `fn` on a float32 array (on the GPU)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    din, dout = DeviceBuffer(max(x.nbytes, 4)).upload(x), DeviceBuffer(max(x.nbytes, 4))
    try:
        check(lib.pt_debug_unary_map(fn, din.ptr, dout.ptr, x.size))
        return dout.download(np.float32, x.shape)
    finally:
        din.free()
        dout.free()


def unary_compare(fn_a, fn_b, first_bits=0, count=1 << 32):
    n, ex = ctypes.c_uint64(0), ctypes.c_uint32(0)
    check(lib.pt_debug_unary_compare(fn_a, fn_b, first_bits, count, ctypes.byref(n), ctypes.byref(ex)))
    return n.value, ex.value

def div_compare(n_first, n_count, first_bits=0, count=1 << 32):
    """Lab library: the kernels' division by a sample count (table reciprocal + exact remainder + one correction) against the
    division itself for counts n_first .. n_first + n_count - 1 and `count` dividend bit patterns from first_bits.
    Returns (mismatches, example dividend bits, example count)."""
    n, ex, exn = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib.pt_debug_div_compare(n_first, n_count, first_bits, count, ctypes.byref(n), ctypes.byref(ex), ctypes.byref(exn)))
    return n.value, ex.value, exn.value


class DeviceBuffer:
    """hipMalloc'd bytes (OutputBuffer::AllocateGPU / Scene's sphere upload)."""

    def __init__(self, nbytes):
        p = _vp()
        check(lib.pt_malloc(ctypes.byref(p), nbytes))
        self.ptr = p.value
        self.nbytes = nbytes

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib.pt_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib.pt_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(lib.pt_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Session:
    """What every ctypes view of a native session shares: the handle, its destroy symbol (`_destroy`, looked up in the loaded
    library), destroy / __del__, and the timed call."""
    handle = None  # (also when __init__ raised before the create)
    _destroy = None

    def destroy(self):
        if self.handle:
            check(getattr(lib, self._destroy)(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _timed(self, fn, *args):
        """fn(handle, *args, &ms): a synchronous entry point whose last argument receives the milliseconds; returns them."""
        ms = ctypes.c_float(0)
        check(fn(self.handle, *args, ctypes.byref(ms)))
        return ms.value

    @staticmethod
    def _lab(name):
        if not IS_LAB:
            raise RuntimeError(f"{name} is a diagnostic of libptcore_lab.so (include/ptcore_lab.h); the product library has none")
        return getattr(lib, name)


class _BatchedStage(_Session):
    """A post-process session whose workspace holds groups of max_frames frames (`_reserve`: its reserve symbol)."""
    _reserve = None

    def reserve_frames(self, n):
        """Workspace for groups of up to n frames (a smaller n is a no-op)."""
        check(getattr(lib, self._reserve)(self.handle, n))
        self.max_frames = max(self.max_frames, n)

    def _strides(self, in_stride, out_stride, in_per_pixel=CHANNELS, out_per_pixel=3):
        """The strides between frames, packed where None: a [H][W][14] frame in, a [H][W][3] image out unless said otherwise."""
        px = self.width * self.height
        return px * in_per_pixel if in_stride is None else in_stride, px * out_per_pixel if out_stride is None else out_stride


@contextlib.contextmanager
def _on_device(*specs, owned=None):
    """The device side of the test conveniences: one DeviceBuffer per spec -- a host array (uploaded), a byte count, or None (no
    buffer: None) -- all freed on exit, also after an exception; `owned`, a session made for the call, is destroyed with them."""
    bufs = []
    try:
        for spec in specs:
            bufs.append(None if spec is None else DeviceBuffer(spec) if isinstance(spec, int) else DeviceBuffer(spec.nbytes).upload(spec))
        yield bufs
    finally:
        for b in bufs:
            if b:
                b.free()
        if owned is not None:
            owned.destroy()


def _ptr(buf):
    return buf.ptr if buf else None


def fast_nearest(spheres, rays, specialised=False, last=False, mask=0xFFFFFFFF):
    """Lab library: the fast mode's nearest<> on rays [n][6] = {o, d} (pt_debug_fast_nearest).  Returns (t float32 [n], index
    int32 [n], -1 for a miss)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = len(rays)
    d_scene, ns = upload_scene(spheres)
    d_rays, d_t, d_idx = DeviceBuffer(max(rays.nbytes, 4)).upload(rays), DeviceBuffer(max(4 * n, 4)), DeviceBuffer(max(4 * n, 4))
    try:
        check(lib.pt_debug_fast_nearest(d_scene.ptr, ns, d_rays.ptr, n, 1 if specialised else 0, 1 if last else 0, mask, d_t.ptr, d_idx.ptr))
        return d_t.download(np.float32, (n,)), d_idx.download(np.int32, (n,))
    finally:
        for b in (d_scene, d_rays, d_t, d_idx):
            b.free()


def policy_ms(rng_mode, variant, waves_per_simd, spp, bounces=5):
    """Lab library: the automatic policy's predicted kernel ms for variant 6 / 8 / 9 on a tile (pt_debug_policy_ms)."""
    ms = ctypes.c_double(0)
    check(lib.pt_debug_policy_ms(rng_mode, variant, waves_per_simd, spp, bounces, ctypes.byref(ms)))
    return ms.value


def policy_choice(rng_mode, waves_per_simd, spp, bounces=5, with9=True):
    """... and the variant the library's OWN policy code (cheapest_variant, csrc/pt_capi.hip) picks from it for the reference's
    scene, in the regime a default renderer is in (samples chunked from 512 spp on): pt_debug_policy_choice."""
    v = ctypes.c_int(0)
    check(lib.pt_debug_policy_choice(rng_mode, waves_per_simd, spp, bounces, 1 if with9 else 0, 1 if spp >= 512 else 0, ctypes.byref(v)))
    return v.value


BUILD_FIELDS = ("flavour", "rng", "kernel", "wide", "lean", "ref", "lanes", "row")
FLAVOUR_PLAIN, FLAVOUR_FRAMES, FLAVOUR_RESUME, FLAVOUR_ADAPTIVE, FLAVOUR_FAST = range(5)
ROW_FIELDS = ("product", "lanes", "threads", "lean", "grid", "wide", "ref_builds", "resume", "frames", "can_chunk", "kernel", "chunk_family")
CENSUS_CHUNKED, CENSUS_REPAIR, CENSUS_PLANAR, CENSUS_VERTICES, CENSUS_RNG_STATE, CENSUS_FOOTPRINT, CENSUS_FIRST_PASS, CENSUS_PRIO = (
    1, 2, 4, 8, 16, 32, 64, 128)


def kernel_builds():
    """Lab library: every distinct kernel function the selectors can return (pt_debug_kernel_builds), one dict of BUILD_FIELDS
    each, in the order launch_census() reports them.  Needs no device."""
    n = ctypes.c_int(0)
    check(lib.pt_debug_kernel_builds(0, ctypes.byref(n), None))
    out = []
    for i in range(n.value):
        info = (ctypes.c_int32 * len(BUILD_FIELDS))()
        check(lib.pt_debug_kernel_builds(i, None, info))
        out.append(dict(zip(BUILD_FIELDS, (int(x) for x in info))))
    return out


def variant_rows():
    """Lab library: the rows of the kernel-variant table (pt_debug_variant_row), one dict of ROW_FIELDS each.  Needs no device."""
    n = ctypes.c_int(0)
    check(lib.pt_debug_variant_row(0, ctypes.byref(n), None))
    out = []
    for i in range(n.value):
        info = (ctypes.c_int32 * len(ROW_FIELDS))()
        check(lib.pt_debug_variant_row(i, None, info))
        out.append(dict(zip(ROW_FIELDS, (int(x) for x in info))))
    return out


def launch_census():
    """Lab library: [(launches, modes)] per build of kernel_builds() since the last launch_census_reset(), plus a last entry for
    launches of functions that are in no build (pt_debug_launch_census; modes = OR of CENSUS_*)."""
    n = ctypes.c_int(0)
    check(lib.pt_debug_kernel_builds(0, ctypes.byref(n), None))
    out = []
    for i in list(range(n.value)) + [-1]:
        launches, modes = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib.pt_debug_launch_census(i, ctypes.byref(launches), ctypes.byref(modes)))
        out.append((launches.value, modes.value))
    return out


def launch_census_reset():
    check(lib.pt_debug_launch_census_reset())


def grid_header(spheres):
    """Diagnostics: the header of kernel variant 11's uniform grid for a scene (pt_debug_grid_header)."""
    d_scene, n = upload_scene(spheres)
    raw = (ctypes.c_uint32 * 16)()
    check(lib.pt_debug_grid_header(d_scene.ptr, n, raw))
    u = np.frombuffer(raw, dtype=np.uint32).copy()
    f = u.view(np.float32)
    return {"valid": int(u[0]), "dims": (int(u[1]), int(u[2]), int(u[3])), "origin": (float(f[4]), float(f[5]), float(f[6])),
            "cell_size": float(f[7]), "slack": float(f[9]), "centre": (float(f[10]), float(f[11]), float(f[12])),
            "far2": float(f[13]), "n_big": int(u[14]) & 0xFFFF, "n_entries": int(u[14]) >> 16, "n_items": int(u[15])}


def grid_image(spheres, eye=None, threads=512):
    """Diagnostics: everything the grid builder writes for a scene (pt_debug_grid_image), decoded: the header fields, the spheres
    outside the grid, per cell the registered spheres (from the cell starts + registration list) and per cell the spheres the
    pooled walk's table lists (inline entries and chained ones followed)."""
    d_scene, n = upload_scene(spheres)
    lay = (ctypes.c_uint64 * 8)()
    check(lib.pt_debug_grid_image(d_scene.ptr, n, None, threads, None, 0, lay))
    raw = (ctypes.c_uint32 * (int(lay[0]) // 4))()
    eye_c = (ctypes.c_float * 3)(*eye) if eye is not None else None
    check(lib.pt_debug_grid_image(d_scene.ptr, n, eye_c, threads, raw, int(lay[0]), lay))
    u = np.frombuffer(raw, dtype=np.uint32).copy()
    f, b = u.view(np.float32), u.view(np.uint8)
    hdr = {"valid": int(u[0]), "dims": (int(u[1]), int(u[2]), int(u[3])), "origin": (float(f[4]), float(f[5]), float(f[6])),
           "cell_size": float(f[7]), "slack": float(f[9]), "centre": (float(f[10]), float(f[11]), float(f[12])), "far2": float(f[13]),
           "n_big": int(u[14]) & 0xFFFF, "n_entries": int(u[14]) >> 16, "n_items": int(u[15]), "r_small": float(f[16]),
           "r_big": float(f[17]), "prim_base": int(u[18]), "n_emis": int(u[19]), "max_entries": int(lay[7])}
    if not hdr["valid"]:
        return hdr
    ncells = hdr["dims"][0] * hdr["dims"][1] * hdr["dims"][2]
    u16 = lambda off, cnt: b[off:off + 2 * cnt].view(np.uint16).astype(np.int64)
    hdr["big"] = u16(int(lay[1]), hdr["n_big"])
    start = u16(int(lay[2]), ncells + 1)
    items = u16(int(lay[3]), hdr["n_items"])
    hdr["cells"] = [items[start[c]:start[c + 1]] for c in range(ncells)]
    tab = b[int(lay[4]):int(lay[4]) + 8 * hdr["n_entries"]].view(np.uint32).reshape(-1, 2)
    pooled = []
    for c in range(ncells):
        got, e = [], c
        for _ in range(hdr["n_entries"] + 1):
            w0, w1 = int(tab[e, 0]), int(tab[e, 1])
            k, link = w0 >> 30, (w0 >> 16) & 0x1FFF
            got += [w0 & 0xFFFF, w1 & 0xFFFF, w1 >> 16][:k]
            if link == 0:
                break
            e = link
        pooled.append(np.asarray(got, dtype=np.int64))
    hdr["pooled"] = pooled
    return hdr


GUARD_WORDS = 64  # sentinel words on either side of every output of the two dumps below
_GUARD = 0xA5A5A5A5


class _Guarded:
    """A device output of `words` 32-bit words between two runs of GUARD_WORDS sentinel words, itself filled with the sentinel."""

    def __init__(self, words):
        self.words = words
        self.buf = DeviceBuffer(4 * (words + 2 * GUARD_WORDS)).upload(np.full(words + 2 * GUARD_WORDS, _GUARD, dtype=np.uint32))
        self.ptr = self.buf.ptr + 4 * GUARD_WORDS

    def finish(self, what):
        """The output words; RuntimeError if a guard word on either side changed."""
        raw = self.buf.download(np.uint32, (self.words + 2 * GUARD_WORDS,))
        if (raw[:GUARD_WORDS] != _GUARD).any() or (raw[GUARD_WORDS + self.words:] != _GUARD).any():
            raise RuntimeError(f"{what}: the guard words around the output were written")
        return raw[GUARD_WORDS:GUARD_WORDS + self.words].copy()


def _primary_dump(spheres, eye, basis, call, outputs):
    """Shared by primary_masks / primary_lists: upload, call(d_scene, n, eye_c, basis_c, *guarded outputs), check the guards and
    that the sphere buffer is what was uploaded."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    d_scene, n = upload_scene(spheres)
    eye_c = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in eye])
    basis_c = (ctypes.c_float * 12)(*[float(v) for v in np.asarray(basis, dtype=np.float32).reshape(12)])
    bufs = [_Guarded(w) if w else None for w in outputs]
    try:
        check(call(d_scene.ptr, n, eye_c, basis_c, *[b.ptr if b else None for b in bufs]))
        got = [b.finish(call.__name__) if b else None for b in bufs]
        if d_scene.download(np.uint8, (spheres.nbytes,)).tobytes() != spheres.tobytes():
            raise RuntimeError(f"{call.__name__}: the sphere buffer changed")
        return got
    finally:
        d_scene.free()
        for b in bufs:
            if b:
                b.buf.free()


def primary_masks(spheres, eye, basis, width, height, row_begin=0, row_end=None, dirs=False):
    """Lab library: primary_candidates (csrc/pt_footprint.h) per pixel of rows [row_begin, row_end), each lane's own word
    (pt_debug_primary_masks): uint32 [pixels]; dirs=True: also the five directions each lane used, float32 [pixels][5][3].
    The outputs lie between guard words and the sphere buffer is read back: RuntimeError if either changed."""
    row_end = height if row_end is None else row_end
    px = max(row_end - row_begin, 0) * width

    def pt_debug_primary_masks(d_scene, n, eye_c, basis_c, d_masks, d_dirs):
        return lib.pt_debug_primary_masks(d_scene, n, eye_c, basis_c, width, height, row_begin, row_end, d_masks, d_dirs)

    masks, d = _primary_dump(spheres, eye, basis, pt_debug_primary_masks, [max(px, 1), 15 * px if dirs else 0])
    masks = masks[:px]
    return (masks, d.view(np.float32).reshape(px, 5, 3)) if dirs else masks


def primary_lists(spheres, eye, basis, width, height, row_begin=0, row_end=None, threads=512):
    """Lab library: build_primary_list (csrc/pt_primlist.h) per LANE of workgroups of `threads` lanes over rows [row_begin,
    row_end) (pt_debug_primary_lists).  Returns (header, lists): header = the grid's 20 header words (word 0 = valid, 16 / 17 the
    bits of r_small / r_big, 14 & 0xFFFF = spheres outside the grid, 18 = prim_base), lists = uint32 [lanes][6] = {valid, length,
    e0.x, e0.y, e1.x, e1.y}, lanes = the tile rounded up to `threads`; None when the grid is invalid (nothing was launched: the
    output must still hold its fill).  Guards and sphere buffer as primary_masks."""
    row_end = height if row_end is None else row_end
    px = max(row_end - row_begin, 0) * width
    lanes = max((px + threads - 1) // threads, 1) * threads
    header = (ctypes.c_uint32 * 20)()

    def pt_debug_primary_lists(d_scene, n, eye_c, basis_c, d_lists):
        return lib.pt_debug_primary_lists(d_scene, n, eye_c, basis_c, width, height, row_begin, row_end, threads, d_lists, header)

    (lists,) = _primary_dump(spheres, eye, basis, pt_debug_primary_lists, [6 * lanes])
    hdr = np.frombuffer(header, dtype=np.uint32).copy()
    if not hdr[0]:
        if (lists != _GUARD).any():
            raise RuntimeError("pt_debug_primary_lists: an invalid grid, yet the output was written")
        return hdr, None
    return hdr, lists.reshape(lanes, 6)


def upload_scene(spheres):
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    return DeviceBuffer(max(spheres.nbytes, 4)).upload(spheres), len(spheres)


class Material(tuple):
    """One sphere's material: Material(kind, param=0.0), a (kind, param) pair like the entries of `materials=[...]`."""

    def __new__(cls, kind, param=0.0):
        return super().__new__(cls, (int(kind), float(param)))

    kind = property(lambda self: self[0])
    param = property(lambda self: self[1])


def material_table(materials):
    """[(kind, param), ...] (or Material objects, or a MATERIAL_DTYPE array) as the pt_material array the library takes."""
    if isinstance(materials, np.ndarray) and materials.dtype == MATERIAL_DTYPE:
        return np.ascontiguousarray(materials)
    rows = [(m, 0.0) if np.isscalar(m) else tuple(m) for m in materials]
    if any(len(r) != 2 for r in rows):
        raise ValueError("materials: every entry is (kind, param)")
    t = np.zeros(len(rows), dtype=MATERIAL_DTYPE)
    for i, (kind, param) in enumerate(rows):
        if int(kind) != kind:
            raise ValueError(f"materials[{i}]: kind {kind!r} is not an integer")
        t[i] = (int(kind), param)
    return t


def material_check(materials):
    """pt_material_check: the host checks of Renderer.set_materials alone (no device); raises PtError naming the entry."""
    t = material_table(materials)
    check(lib.pt_material_check(t.ctypes.data if len(t) else None, len(t)))


class PtSky(ctypes.Structure):
    """pt_sky (include/ptcore.h)."""
    _fields_ = [("zenith", ctypes.c_float * 3), ("horizon", ctypes.c_float * 3), ("ground", ctypes.c_float * 3),
                ("sun_dir", ctypes.c_float * 3), ("sun_cos", ctypes.c_float), ("sun_radiance", ctypes.c_float * 3)]


class Sky:
    """A sky and, optionally, a sun (pt_sky, EXACTNESS.md A.24): radiance `zenith` straight up, `horizon` at the horizon, `ground`
    for every direction below it (world up is +y); a sun of radiance `sun_radiance` wherever the angle to `sun_dir` (towards the
    sun, any length) has a cosine of at least `sun_cos`.  Without sun_radiance (or all zero) there is no sun."""

    def __init__(self, zenith, horizon, ground, sun_dir=None, sun_cos=None, sun_radiance=None):
        vec = lambda v: tuple(float(x) for x in ((0.0, 0.0, 0.0) if v is None else v))  # noqa: E731
        self.zenith, self.horizon, self.ground = vec(zenith), vec(horizon), vec(ground)
        self.sun_dir, self.sun_radiance = vec(sun_dir), vec(sun_radiance)
        self.sun_cos = 0.0 if sun_cos is None else float(sun_cos)
        for name in ("zenith", "horizon", "ground", "sun_dir", "sun_radiance"):
            if len(getattr(self, name)) != 3:
                raise ValueError(f"Sky: {name} takes three components")

    def as_struct(self):
        return PtSky(self.zenith, self.horizon, self.ground, self.sun_dir, self.sun_cos, self.sun_radiance)

    def as_dict(self):
        """The description as tests/sky_model.py takes it."""
        return {k: getattr(self, k) for k in ("zenith", "horizon", "ground", "sun_dir", "sun_cos", "sun_radiance")}

    def __repr__(self):
        return "Sky(%r, %r, %r, sun_dir=%r, sun_cos=%r, sun_radiance=%r)" % (self.zenith, self.horizon, self.ground, self.sun_dir, self.sun_cos,
                                                                           self.sun_radiance)


# a clear day: a blue-to-white gradient, a grey ground and a sun of angular radius 2.56 degrees (cos 0.999, 0.0063 sr) 64 degrees
# above the horizon whose radiance is 500 to 1000 times the sky's
CLEAR_SKY = Sky(zenith=(0.18, 0.36, 0.80), horizon=(0.80, 0.85, 0.90), ground=(0.25, 0.25, 0.25), sun_dir=(0.4, 0.8, 0.45), sun_cos=0.999,
                sun_radiance=(400.0, 380.0, 340.0))


def sky_check(sky):
    """pt_sky_check: the host checks of Renderer.set_sky alone (no device); raises PtError naming the field."""
    if sky is None:
        check(lib.pt_sky_check(None))
        return
    st = sky.as_struct()
    check(lib.pt_sky_check(ctypes.addressof(st)))


class Renderer(_Session):
    """ctypes view of pt_renderer (the reference's class Renderer, include/Renderer.h)."""
    _destroy = "pt_renderer_destroy"

    def __init__(self, width, height, spp, threads_per_block=8, *, max_bounces=5, rng_mode=RNG_XORWOW, seed=0,
                 row_begin=0, row_end=0, persist_rng=True, variant=None, layout=LAYOUT_INTERLEAVED, fast_math=False, chunks=0):
        o = RendererOpts()
        lib.pt_renderer_opts_default(ctypes.byref(o))
        o.max_bounces, o.rng_mode, o.seed = max_bounces, rng_mode, seed
        o.row_begin, o.row_end = row_begin, row_end
        o.persist_rng = 1 if persist_rng else 0
        o.layout = layout
        o.fast_math = 1 if fast_math else 0
        o.chunks = chunks  # 0 automatic, 1 off, n >= 2 chunks
        if variant is not None:
            o.variant = variant
        self.variant = o.variant
        h = _vp()
        check(lib.pt_renderer_create(width, height, spp, threads_per_block, ctypes.byref(o), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height, self.spp = width, height, spp
        self.row_begin = row_begin
        self.row_end = row_end if (row_begin or row_end) else height
        self.rows = self.row_end - self.row_begin

    @property
    def tile_floats(self):
        return self.rows * self.width * CHANNELS

    def render(self, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE):
        """Synchronous Render(); returns kernel milliseconds (Renderer.h:55-76)."""
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        return self._timed(lib.pt_renderer_render, d_out, d_spheres, n_spheres, b, e)

    def enqueue(self, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE, stream=None):
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        check(lib.pt_renderer_enqueue(self.handle, d_out, d_spheres, n_spheres, b, e, stream))

    def enqueue_frames(self, d_out, out_stride_floats, d_spheres, n_spheres, bases, eyes, d_vertices=None, vtx_stride_floats=0, stream=None):
        """n frames of known cameras (bases [n][12], eyes [n][3]) into d_out + f * out_stride_floats: pt_renderer_enqueue_frames."""
        bases = np.ascontiguousarray(bases, dtype=np.float32).reshape(-1, 12)
        eyes = np.ascontiguousarray(eyes, dtype=np.float32).reshape(-1, 3)
        assert len(bases) == len(eyes)
        check(lib.pt_renderer_enqueue_frames(self.handle, len(bases), d_out, out_stride_floats, d_vertices, vtx_stride_floats, d_spheres,
                                             n_spheres, bases.ctypes.data_as(_fp), eyes.ctypes.data_as(_fp), stream))

    def check(self, wait=True):
        """Status of the frames enqueued so far (raises PtError(PT_EKERNEL) for a frame whose sample-chunk chain broke);
        returns the number of frames render() has repaired in place."""
        n = ctypes.c_uint32(0)
        check(lib.pt_renderer_check(self.handle, 1 if wait else 0, ctypes.byref(n)))
        return n.value

    def set_display(self, d_vertices):
        """Every frame also writes the display vertices (Denoiser::Denoise fused into the render); None switches it off."""
        check(lib.pt_renderer_set_display(self.handle, d_vertices))

    def set_materials(self, materials):
        """One (kind, param) per sphere: from now on every frame runs the materials kernel (kernel_info: VARIANT_MATERIALS).
        None clears the table: the ordinary kernels again, bit for bit."""
        if materials is None:
            check(lib.pt_renderer_set_materials(self.handle, None, 0))
            return
        t = material_table(materials)
        check(lib.pt_renderer_set_materials(self.handle, t.ctypes.data if len(t) else None, len(t)))

    def set_light_sampling(self, on):
        """Direct light sampling (next-event estimation, EXACTNESS.md A.23): every DIFFUSE hit but the last bounce's samples each
        emitting sphere (kernel_info: VARIANT_MATERIALS_LIGHTS), with or without a material table.  False: exactly what the
        renderer was before."""
        check(lib.pt_renderer_set_light_sampling(self.handle, 1 if on else 0))

    def set_sky(self, sky):
        """A Sky (EXACTNESS.md A.24): from now on an escaping path takes the sky's radiance and every frame runs a SKY build of the
        materials kernel (kernel_info: VARIANT_MATERIALS_SKY, or VARIANT_MATERIALS_LIGHTS_SKY with light sampling, which then
        samples the sun as its last light), with or without a material table.  None clears it: exactly what the renderer was."""
        if sky is None:
            check(lib.pt_renderer_set_sky(self.handle, None))
            return
        st = sky.as_struct()
        check(lib.pt_renderer_set_sky(self.handle, ctypes.addressof(st)))

    def set_frame(self, frame):
        check(lib.pt_renderer_set_frame(self.handle, frame))

    def reset_rng(self):
        check(lib.pt_renderer_reset_rng(self.handle))

    def get_rng_state(self):
        st = np.zeros((self.rows * self.width, 6), dtype=np.uint32)
        check(lib.pt_renderer_get_rng_state(self.handle, st.ctypes.data, st.size))
        return st

    def set_rng_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.uint32)
        check(lib.pt_renderer_set_rng_state(self.handle, st.ctypes.data, st.size))

    def batch_launches(self):  # lab library only (pt_debug_renderer_batch_launches)
        """Launches of the frames kernel that enqueue_frames has made on this renderer (single enqueues do not count)."""
        n = ctypes.c_uint32(0)
        check(lib.pt_debug_renderer_batch_launches(self.handle, ctypes.byref(n)))
        return n.value

    def kernel_info(self, n_spheres):
        ki = KernelInfo()
        check(lib.pt_renderer_kernel_info(self.handle, n_spheres, ctypes.byref(ki)))
        return {f: getattr(ki, f) for f, _ in KernelInfo._fields_ if not f.startswith("reserved")}


class Progressive(_Session):
    """ctypes view of pt_progressive: one still frame of `renderer` refined pass by pass (include/ptcore.h).  After a pass that
    leaves the session at n >= 2 samples the frame equals the first Render() of a fresh renderer at n spp, bit for bit."""
    _destroy = "pt_progressive_destroy"

    def __init__(self, renderer):
        h = _vp()
        check(lib.pt_progressive_create(renderer.handle, ctypes.byref(h)))
        self.handle = h.value
        self.renderer = renderer  # (the session uses the renderer's scratch: keep it alive)

    def enqueue(self, spp, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE, stream=None):
        """Asynchronous pass of spp samples; d_out receives the frame of all samples so far."""
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        check(lib.pt_progressive_enqueue(self.handle, spp, d_out, d_spheres, n_spheres, b, e, stream))

    def render(self, spp, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE):
        """Synchronous pass; returns device-event milliseconds."""
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        return self._timed(lib.pt_progressive_render, spp, d_out, d_spheres, n_spheres, b, e)

    def samples(self):
        n = ctypes.c_int64(0)
        check(lib.pt_progressive_samples(self.handle, ctypes.byref(n)))
        return n.value

    def reset(self):
        check(lib.pt_progressive_reset(self.handle))

    def variant(self, n_spheres):
        """The kernel variant the next pass on a scene of n_spheres runs (6, 10, 13 or 14)."""
        v = ctypes.c_int(0)
        check(lib.pt_progressive_variant(self.handle, n_spheres, ctypes.byref(v)))
        return v.value

    def set_samples(self, n):  # lab library only (pt_debug_progressive_set_samples)
        check(lib.pt_debug_progressive_set_samples(self.handle, n))

    def set_adaptive(self, tolerance, floor=ADAPTIVE_FLOOR, min_samples=ADAPTIVE_MIN_SAMPLES, radius=ADAPTIVE_RADIUS):
        """Adaptive sampling from the next first pass on (only at 0 samples): pixels whose mean luminance has a relative
        standard error <= tolerance stop (include/ptcore.h has the rule).  tolerance=None turns it off."""
        if tolerance is None:
            check(lib.pt_progressive_set_adaptive(self.handle, None))
            return
        o = AdaptiveOpts(float(tolerance), float(floor), int(min_samples), int(radius))
        check(lib.pt_progressive_set_adaptive(self.handle, ctypes.byref(o)))

    def active(self):
        """How many pixels the next pass renders (synchronous)."""
        n = ctypes.c_int64(0)
        check(lib.pt_progressive_active(self.handle, ctypes.byref(n)))
        return n.value

    def counts(self):
        """Every tile pixel's sample count, an int32 torch tensor on the current device (tile order)."""
        import torch

        n = self.renderer.rows * self.renderer.width
        t = torch.empty(n, dtype=torch.int32, device="cuda")
        if n:
            torch.cuda.synchronize()
            check(lib.pt_progressive_counts(self.handle, t.data_ptr(), None))
            torch.cuda.synchronize()
        return t

    def refine(self, max_samples, pass_spp, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE, on_pass=None):
        """Synchronous passes of pass_spp samples until no pixel is active or the next pass would take the session past
        max_samples per pixel.  on_pass(session, pass_index, ms) is called after every pass.  Returns the number of passes."""
        passes = 0
        while not (passes > 0 and self.active() == 0) and self.samples() + pass_spp <= max_samples:
            ms = self.render(pass_spp, d_out, d_spheres, n_spheres, basis, eye)
            if on_pass is not None:
                on_pass(self, passes, ms)
            passes += 1
        return passes

    def record(self):  # lab library only (pt_debug_progressive_record): [26][tile pixels] uint32
        n = self.renderer.rows * self.renderer.width
        a = np.zeros((REC_WORDS, n), dtype=np.uint32)
        check(lib.pt_debug_progressive_record(self.handle, a.ctypes.data))
        return a

    def set_active(self, mask):  # lab library only (pt_debug_progressive_set_active)
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        check(lib.pt_debug_progressive_set_active(self.handle, m.ctypes.data))


def debug_adaptive_select(rec, width, n, n_end, mode, peek, tolerance, floor, min_samples, radius, mask, counts, lst, words):
    """Lab library only (pt_debug_adaptive_select): the selection kernels of an adaptive pass on host arrays.  rec [26][pixels]
    uint32; mask uint8, counts and lst uint32 of `pixels` entries, words uint32 of 2.  Nothing is changed in place: returns
    (mask, counts, list, words, block prefix) as the call left them."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    tp = rec.shape[1]
    assert rec.shape[0] == REC_WORDS
    out = [np.array(a, dtype=t, copy=True).reshape(-1) for a, t in ((mask, np.uint8), (counts, np.uint32), (lst, np.uint32), (words, np.uint32))]
    assert [a.size for a in out] == [tp, tp, tp, 2]
    sums = np.zeros((tp + 255) // 256, dtype=np.uint32)
    o = AdaptiveOpts(float(tolerance), float(floor), int(min_samples), int(radius))
    check(lib.pt_debug_adaptive_select(rec.ctypes.data, tp, int(width), int(n), int(n_end), int(mode), int(bool(peek)), ctypes.byref(o),
                                       out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, sums.ctypes.data))
    return out[0], out[1], out[2], out[3], sums


def debug_adaptive_finalize(rec, counts, planar):
    """Lab library only (pt_debug_adaptive_finalize): the frame of rec [26][pixels] at counts [pixels], float32 [pixels][14] or,
    planar, [14][pixels]."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    tp = rec.shape[1]
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    assert rec.shape[0] == REC_WORDS and counts.size == tp
    out = np.zeros((14, tp) if planar else (tp, 14), dtype=np.float32)
    check(lib.pt_debug_adaptive_finalize(rec.ctypes.data, counts.ctypes.data, tp, int(bool(planar)), out.ctypes.data))
    return out


class MultiRenderer(_Session):
    """ctypes view of pt_mgpu: one frame row-tiled over several devices of this process (one host thread per
    device inside the library, RCCL or peer-copy exchange to devices[0])."""
    _destroy = "pt_mgpu_destroy"

    def __init__(self, devices, width, height, spp, threads_per_block=8, *, max_bounces=5, rng_mode=RNG_XORWOW, seed=0,
                 persist_rng=True, variant=None, gather=None, force_exchange=None, timeout_ms=None, fast_math=False, bands=None):
        o = RendererOpts()
        lib.pt_renderer_opts_default(ctypes.byref(o))
        o.max_bounces, o.rng_mode, o.seed = max_bounces, rng_mode, seed
        o.persist_rng = 1 if persist_rng else 0
        o.fast_math = 1 if fast_math else 0
        if variant is not None:
            o.variant = variant
        mo = MgpuOpts()
        lib.pt_mgpu_opts_default(ctypes.byref(mo))
        if gather is not None:
            mo.gather = gather
        if force_exchange is not None:
            mo.force_exchange = 1 if force_exchange else 0
        if timeout_ms is not None:
            mo.timeout_ms = timeout_ms
        if bands is not None:
            mo.bands = bands  # 0 automatic, n row bands per tile (pipelined exchange)
        devs = (ctypes.c_int * len(devices))(*devices)
        h = _vp()
        check(lib.pt_mgpu_create(len(devices), devs, width, height, spp, threads_per_block, ctypes.byref(o), ctypes.byref(mo), ctypes.byref(h)))
        self.handle = h.value
        self.n, self.width, self.height, self.spp = len(devices), width, height, spp

    def render(self, d_out, d_spheres, n_spheres, basis, eye=DEFAULT_EYE):
        """Synchronous; returns end-to-end wall milliseconds (render + exchange)."""
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        return self._timed(lib.pt_mgpu_render, d_out, d_spheres, n_spheres, b, e)

    def tile(self, rank):
        dev, rb, re_, ms = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_float(0)
        check(lib.pt_mgpu_tile(self.handle, rank, ctypes.byref(dev), ctypes.byref(rb), ctypes.byref(re_), ctypes.byref(ms)))
        return {"rank": rank, "device": dev.value, "rows": (rb.value, re_.value), "kernel_ms": ms.value}

    def frame_stats(self):
        """Last frame: bands per tile, the longest rank's render ms, and what the exchange added on top (wall - render)."""
        b, r, x = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_float(0)
        check(lib.pt_mgpu_frame_stats(self.handle, ctypes.byref(b), ctypes.byref(r), ctypes.byref(x)))
        return {"bands": b.value, "render_ms": r.value, "exposed_ms": x.value}

    def backend(self):
        buf = ctypes.create_string_buffer(128)
        check(lib.pt_mgpu_backend(self.handle, buf, 128))
        return buf.value.decode()


def render_frame(width, height, spp, spheres=None, basis=None, eye=DEFAULT_EYE, materials=None, light_sampling=False, sky=None, **opts):
    """Convenience for tests: allocate, render rows [row_begin,row_end) on the GPU, download.
    Returns (float32 [rows][width][14], kernel_ms).  materials: [(kind, param), ...], one per sphere (Renderer.set_materials);
    light_sampling: Renderer.set_light_sampling; sky: a Sky (Renderer.set_sky)."""
    if spheres is None:
        spheres = scene_cornell()
    if basis is None:
        basis = camera_basis(eye, width=width, height=height)
    if materials is not None:
        material_check(materials)  # before a renderer (a device) exists
    if sky is not None:
        sky_check(sky)
    r = Renderer(width, height, spp, **opts)
    d_scene, n = upload_scene(spheres)
    d_out = DeviceBuffer(max(r.tile_floats * 4, 4))
    try:
        if materials is not None:
            r.set_materials(materials)
        if light_sampling:
            r.set_light_sampling(True)
        if sky is not None:
            r.set_sky(sky)
        ms = r.render(d_out.ptr, d_scene.ptr, n, basis, eye)
        img = d_out.download(np.float32, (r.rows, width, CHANNELS))
    finally:
        d_out.free()
        d_scene.free()
        r.destroy()
    return img, ms


def denoiser_weights_bytes(weights):
    """PTDN bytes from a path, bytes or a reference-keyed state_dict (denoise_weights.py)."""
    if isinstance(weights, (bytes, bytearray, memoryview)):
        return bytes(weights)
    if isinstance(weights, (str, os.PathLike)):
        with open(weights, "rb") as f:
            return f.read()
    from . import denoise_weights

    return denoise_weights.to_bytes(weights)


def denoiser_weights_check(weights):
    """Host-only validation of a weight file / bytes / state_dict (pt_denoiser_weights_check); raises PtError naming the key."""
    blob = denoiser_weights_bytes(weights)
    check(lib.pt_denoiser_weights_check(blob, len(blob)))


DENOISE_F32, DENOISE_F16 = 0, 1
_DENOISE_PRECISIONS = {"float32": DENOISE_F32, "half": DENOISE_F16}


class DenoiserOpts(ctypes.Structure):
    """pt_denoiser_opts (include/ptcore.h)."""
    _fields_ = [("precision", ctypes.c_int32), ("max_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def denoise_precision(precision):
    """PT_DENOISE_* of a precision name ("float32" or "half"); anything else is a ValueError."""
    if precision not in _DENOISE_PRECISIONS:
        raise ValueError(f"precision {precision!r}: 'float32' or 'half'")
    return _DENOISE_PRECISIONS[precision]


class Denoiser(_BatchedStage):
    """ctypes view of pt_denoiser: the reference's DenoiseCNN step (train.py:test, main.cu:146-152) for width x height frames.
    weights: a PTDN file path, its bytes, or a reference-keyed state_dict.  max_frames > 1 reserves the workspace for batches
    of that many frames per group (pt_denoiser_reserve_frames).  precision: "float32" (the default, exact to fp32 rounding)
    or "half" (fp16 operands and storage, fp32 accumulation: the toleranced mode of DENOISER.md, "Half precision")."""
    _destroy, _reserve = "pt_denoiser_destroy", "pt_denoiser_reserve_frames"

    def __init__(self, width, height, weights, max_frames=1, precision="float32"):
        opts = DenoiserOpts(precision=denoise_precision(precision), max_frames=max_frames)
        blob = denoiser_weights_bytes(weights)
        h = _vp()
        check(lib.pt_denoiser_create_opts(width, height, blob, len(blob), ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height = width, height
        self.max_frames = max_frames

    @property
    def precision(self):
        """"float32" or "half" (pt_denoiser_precision)."""
        v = ctypes.c_int(-1)
        check(lib.pt_denoiser_precision(self.handle, ctypes.byref(v)))
        return {n: k for k, n in _DENOISE_PRECISIONS.items()}[v.value]

    def enqueue_frames(self, d_frames, n, frame_stride_floats=None, d_rgb=None, rgb_stride_floats=None, stream=None):
        """Asynchronous; n frames at d_frames + f * frame_stride_floats (default: packed [n][H][W][14]), in place or, with d_rgb,
        [H][W][3] at d_rgb + f * rgb_stride_floats (default packed): bit for bit n single enqueues."""
        fs, rs = self._strides(frame_stride_floats, rgb_stride_floats)
        check(lib.pt_denoiser_enqueue_frames(self.handle, n, d_frames, fs, d_rgb, rs, stream))

    def denoise_frames(self, d_frames, n, frame_stride_floats=None, d_rgb=None, rgb_stride_floats=None):
        """Synchronous enqueue_frames; returns device-event milliseconds."""
        fs, rs = self._strides(frame_stride_floats, rgb_stride_floats)
        return self._timed(lib.pt_denoiser_denoise_frames, n, d_frames, fs, d_rgb, rs)

    def enqueue(self, d_frame, d_rgb=None, stream=None):
        """Asynchronous; d_rgb None = in place on the [H][W][14] frame, else [H][W][3] into d_rgb (frame untouched)."""
        check(lib.pt_denoiser_enqueue(self.handle, d_frame, d_rgb, stream))

    def denoise(self, d_frame, d_rgb=None):
        """Synchronous; returns device-event milliseconds."""
        return self._timed(lib.pt_denoiser_denoise, d_frame, d_rgb)

    # lab library only (pt_debug_denoiser_*)
    def layers(self):
        """[(name, (rows, cols, channels))] of every activation buffer of the workspace."""
        n, shape, name = ctypes.c_int(0), (ctypes.c_int * 3)(), ctypes.create_string_buffer(64)
        check(lib.pt_debug_denoiser_layer_info(self.handle, 0, ctypes.byref(n), shape, name, 64))
        out = []
        for i in range(n.value):
            check(lib.pt_debug_denoiser_layer_info(self.handle, i, None, shape, name, 64))
            out.append((name.value.decode(), tuple(shape)))
        return out

    def activation(self, layer, frames=None):
        """Layer `layer` of the first frame, [rows][cols][channels]; frames=g: of the first g frames, [g][rows][cols][channels]."""
        shape = self.layers()[layer][1]
        if frames is None:
            out = np.empty(shape, dtype=np.float32)
            check(lib.pt_debug_denoiser_activation(self.handle, layer, out.ctypes.data, out.size))
        else:
            out = np.empty((max(frames, 0),) + shape, dtype=np.float32)
            check(lib.pt_debug_denoiser_activation_frames(self.handle, layer, frames, out.ctypes.data, out.size))
        return out

    def set_activation(self, layer, arr, frames=None):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if frames is None:
            check(lib.pt_debug_denoiser_set_activation(self.handle, layer, arr.ctypes.data, arr.size))
        else:
            check(lib.pt_debug_denoiser_set_activation_frames(self.handle, layer, frames, arr.ctypes.data, arr.size))

    def convs(self):
        """[(name, info dict)] of every convolution in execution order (pt_debug_denoiser_conv_info)."""
        n, info, name = ctypes.c_int(0), (ctypes.c_int * 12)(), ctypes.create_string_buffer(64)
        check(lib.pt_debug_denoiser_conv_info(self.handle, 0, ctypes.byref(n), info, name, 64))
        keys = ("in", "out0", "out1", "res", "up", "ks", "stride", "N", "epi", "splits", "bm", "bn")
        out = []
        for i in range(n.value):
            check(lib.pt_debug_denoiser_conv_info(self.handle, i, None, info, name, 64))
            out.append((name.value.decode(), dict(zip(keys, list(info)))))
        return out

    def run_conv(self, conv, d_out=None, frames=None, ld=3, frame_stride=None):
        """Convolution `conv` alone, synchronous.  frames=g: of the plan of a group of g frames, on the first g frames of the
        workspace; the head writes d_out[f * frame_stride + pixel * ld + (0 .. 2)] (frame_stride in floats, default packed)."""
        if frames is None:
            check(lib.pt_debug_denoiser_run_conv(self.handle, conv, d_out))
        else:
            fs = self.width * self.height * ld if frame_stride is None else frame_stride
            check(lib.pt_debug_denoiser_run_conv_frames(self.handle, conv, d_out, frames, ld, fs))

    def run_pre(self, d_frames, frames, frame_stride=None, inplace=True):
        """The pre-processing of a group of `frames` frames alone, synchronous (frame_stride in floats, default packed)."""
        fs = self.width * self.height * CHANNELS if frame_stride is None else frame_stride
        check(lib.pt_debug_denoiser_run_pre(self.handle, d_frames, frames, fs, 1 if inplace else 0))

    def memory(self):
        """Bytes (pt_debug_denoiser_memory): {"element", "workspace", "partials", "weights", "layers": [(name, offset, bytes
        of one frame)]}."""
        info = (ctypes.c_uint64 * 6)()
        layers = []
        for i, (name, _) in enumerate(self.layers()):
            check(lib.pt_debug_denoiser_memory(self.handle, i, info))
            layers.append((name, int(info[1]), int(info[2])))
        return {"element": int(info[0]), "workspace": int(info[3]), "partials": int(info[4]), "weights": int(info[5]),
                "layers": layers}

    def last_enqueue(self):
        """(groups, kernel launches) of the last enqueue (pt_debug_denoiser_last_enqueue)."""
        g, n = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.pt_debug_denoiser_last_enqueue(self.handle, ctypes.byref(g), ctypes.byref(n)))
        return g.value, n.value

    def conv_plan(self, n_frames):
        """[info dict] of every convolution in the plan of a group of n_frames frames (pt_debug_denoiser_conv_plan)."""
        info = (ctypes.c_int * 6)()
        keys = ("M", "bm", "bn", "splits", "chunks_per_split", "workgroups")
        out = []
        for i in range(len(self.convs())):
            check(lib.pt_debug_denoiser_conv_plan(self.handle, n_frames, i, info))
            out.append(dict(zip(keys, list(info))))
        return out


def denoise_frame(frame, weights, out_of_place=False, denoiser=None, precision="float32"):
    """Convenience for tests: upload a host [H][W][14] frame, denoise it on the GPU, download.  Returns the frame after the
    in-place step, or (frame untouched, rgb [H][W][3]) with out_of_place=True.  precision: of the denoiser made here."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[:2]
    dn = denoiser or Denoiser(w, h, weights, precision=precision)
    with _on_device(frame, h * w * 12 if out_of_place else None, owned=None if denoiser else dn) as (d_frame, d_rgb):
        dn.denoise(d_frame.ptr, _ptr(d_rgb))
        f = d_frame.download(np.float32, frame.shape)
        return (f, d_rgb.download(np.float32, (h, w, 3))) if out_of_place else f


def denoise_frames(frames, weights, out_of_place=False, denoiser=None, precision="float32"):
    """The batched twin of denoise_frame: host frames [N][H][W][14] through ONE pt_denoiser_denoise_frames call (a denoiser
    reserved for all N frames unless one is given).  Returns the frames after the in-place step, or (frames untouched,
    rgb [N][H][W][3]) with out_of_place=True."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    n, h, w = frames.shape[:3]
    dn = denoiser or Denoiser(w, h, weights, max_frames=n, precision=precision)
    with _on_device(frames, n * h * w * 12 if out_of_place else None, owned=None if denoiser else dn) as (d_frames, d_rgb):
        dn.denoise_frames(d_frames.ptr, n, d_rgb=_ptr(d_rgb))
        f = d_frames.download(np.float32, frames.shape)
        return (f, d_rgb.download(np.float32, (n, h, w, 3))) if out_of_place else f


class FilterOpts(ctypes.Structure):
    """pt_filter_opts (include/ptcore.h)."""
    _fields_ = [("iterations", ctypes.c_int32), ("sigma_l", ctypes.c_float), ("sigma_n", ctypes.c_float), ("sigma_a", ctypes.c_float),
                ("sigma_z", ctypes.c_float), ("max_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class FilterSpatialOpts(ctypes.Structure):
    """pt_filter_spatial_opts (include/ptcore.h)."""
    _fields_ = [("below", ctypes.c_uint32), ("radius", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


FILTER_SPATIAL_ALL = 0xFFFFFFFF  # PT_FILTER_SPATIAL_ALL: every pixel takes the estimate


def _filter_spatial_opts(below, radius, reserved=(0, 0)):
    if below == "all":
        below = FILTER_SPATIAL_ALL
    if not 0 <= int(below) <= FILTER_SPATIAL_ALL:
        raise ValueError(f"spatial_below {below} outside 0 .. 2^32 - 1")
    o = FilterSpatialOpts(below=int(below), radius=radius)
    o.reserved[0], o.reserved[1] = reserved
    return o


def filter_spatial_check(below, radius=2, reserved=(0, 0)):
    """pt_filter_spatial_check: the host checks of FeatureFilter.set_spatial alone; host only.  Raises PtError for what it refuses."""
    check(lib.pt_filter_spatial_check(ctypes.byref(_filter_spatial_opts(below, radius, reserved))))


class FeatureFilter(_BatchedStage):
    """ctypes view of pt_filter: the weights-free denoiser for width x height frames, a variance-guided edge-avoiding a-trous
    filter on albedo-demodulated colour (DENOISER.md, "Feature-guided filter").  max_frames > 1 reserves the workspace for
    batches of that many frames per group.  samples: the frame's count per pixel; d_counts: a device uint32 [H][W] count image
    (Progressive.counts' layout) that replaces it.  spatial_below > 0 (or "all"): the spatial variance estimate for the pixels
    with fewer samples than that, over a (2 spatial_radius + 1)^2 window (set_spatial)."""
    _destroy, _reserve = "pt_filter_destroy", "pt_filter_reserve_frames"

    def __init__(self, width, height, max_frames=1, iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0, spatial_below=0,
                 spatial_radius=2):
        opts = FilterOpts(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_a=sigma_a, sigma_z=sigma_z, max_frames=max_frames)
        spatial = _filter_spatial_opts(spatial_below, spatial_radius)
        if spatial.below != 0:  # (refused here, before a filter exists)
            check(lib.pt_filter_spatial_check(ctypes.byref(spatial)))
        h = _vp()
        check(lib.pt_filter_create(width, height, ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height = width, height
        self.max_frames = max_frames
        self.iterations = iterations
        if spatial.below != 0:
            self.set_spatial(spatial_below, spatial_radius)

    def set_spatial(self, below, radius=2):
        """pt_filter_set_spatial: the spatial variance estimate (DENOISER.md, "Spatial variance estimate") for the pixels with
        fewer than `below` samples ("all": every pixel; 0 or None: off), window (2 radius + 1)^2.  Holds for later calls."""
        if below is None:
            check(lib.pt_filter_set_spatial(self.handle, None))
        else:
            check(lib.pt_filter_set_spatial(self.handle, ctypes.byref(_filter_spatial_opts(below, radius))))

    def memory(self):
        """{"workspace": bytes of the state and guide images of all max_frames frames, "per_pixel": bytes per pixel and frame}."""
        b = ctypes.c_uint64(0)
        check(lib.pt_filter_workspace_bytes(self.handle, ctypes.byref(b)))
        return {"workspace": int(b.value), "per_pixel": int(b.value) // (self.max_frames * self.width * self.height)}

    def enqueue(self, d_frame, samples, d_rgb=None, d_counts=None, stream=None):
        """Asynchronous; d_rgb None = in place on the [H][W][14] frame, else [H][W][3] into d_rgb (frame untouched)."""
        check(lib.pt_filter_enqueue(self.handle, d_frame, d_rgb, samples, d_counts, stream))

    def run(self, d_frame, samples, d_rgb=None, d_counts=None):
        """Synchronous; returns device-event milliseconds."""
        return self._timed(lib.pt_filter_run, d_frame, d_rgb, samples, d_counts)

    def enqueue_frames(self, d_frames, n, samples, frame_stride_floats=None, d_rgb=None, rgb_stride_floats=None, stream=None):
        """Asynchronous; n frames at d_frames + k * frame_stride_floats (default: packed [n][H][W][14]), in place or, with d_rgb,
        [H][W][3] at d_rgb + k * rgb_stride_floats (default packed): bit for bit n single enqueues."""
        fs, rs = self._strides(frame_stride_floats, rgb_stride_floats)
        check(lib.pt_filter_enqueue_frames(self.handle, n, d_frames, fs, d_rgb, rs, samples, stream))

    def run_frames(self, d_frames, n, samples, frame_stride_floats=None, d_rgb=None, rgb_stride_floats=None):
        """Synchronous enqueue_frames; returns device-event milliseconds."""
        fs, rs = self._strides(frame_stride_floats, rgb_stride_floats)
        return self._timed(lib.pt_filter_run_frames, n, d_frames, fs, d_rgb, rs, samples)

    def step(self, d_frame, samples, step, d_rgb=None, d_counts=None):
        """Lab library only: the set-up and one iteration at `step`, fused with the re-modulation; synchronous."""
        check(self._lab("pt_debug_filter_step")(self.handle, d_frame, d_rgb, samples, d_counts, step))

    def tiled(self, on):
        """Lab library only: steps 1 and 2 through the LDS tile (True) or with direct loads (False)."""
        check(self._lab("pt_debug_filter_tiled")(self.handle, int(bool(on))))

    def state(self, d_frame, samples, steps=(), d_counts=None):
        """Lab library only: the set-up and one UNFUSED iteration per entry of `steps` (none: the set-up alone) on the device
        frame; returns host copies (state {ill.rgb, var}, guide {n.xyz, z}, guide {alb.rgb, dz}), each [H][W][4] float32."""
        steps = [int(s) for s in steps]
        arr = (ctypes.c_int * max(len(steps), 1))(*steps)
        nbytes = self.width * self.height * 16
        bufs = [DeviceBuffer(nbytes) for _ in range(3)]
        try:
            check(self._lab("pt_debug_filter_state")(self.handle, d_frame, samples, d_counts, arr, len(steps), *(b.ptr for b in bufs)))
            return tuple(b.download(np.float32, (self.height, self.width, 4)) for b in bufs)
        finally:
            for b in bufs:
                b.free()


def filter_frame(frame, samples, out_of_place=False, filt=None, counts=None, spatial_below=None, spatial_radius=2, **opts):
    """Convenience for tests: upload a host [H][W][14] frame, filter it on the GPU, download.  Returns the frame after the
    in-place step, or (frame untouched, rgb [H][W][3]) with out_of_place=True.  counts: a host uint32 [H][W] count image.
    spatial_below, spatial_radius: FeatureFilter.set_spatial before the run (it holds on a `filt` passed in).
    opts: of the FeatureFilter made here (iterations, sigma_*)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[:2]
    ff = filt or FeatureFilter(w, h, spatial_below=spatial_below or 0, spatial_radius=spatial_radius, **opts)
    if filt and spatial_below is not None:
        filt.set_spatial(spatial_below, spatial_radius)
    counts = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    with _on_device(frame, h * w * 12 if out_of_place else None, counts, owned=None if filt else ff) as (d_frame, d_rgb, d_counts):
        ff.run(d_frame.ptr, samples, _ptr(d_rgb), _ptr(d_counts))
        f = d_frame.download(np.float32, frame.shape)
        return (f, d_rgb.download(np.float32, (h, w, 3))) if out_of_place else f


def filter_frames(frames, samples, out_of_place=False, filt=None, spatial_below=None, spatial_radius=2, **opts):
    """The batched twin of filter_frame: host frames [N][H][W][14] through ONE pt_filter_run_frames call (a filter reserved
    for all N frames unless one is given).  Returns the frames after the in-place step, or (frames untouched, rgb
    [N][H][W][3]) with out_of_place=True.  spatial_below, spatial_radius: as filter_frame."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    n, h, w = frames.shape[:3]
    ff = filt or FeatureFilter(w, h, max_frames=n, spatial_below=spatial_below or 0, spatial_radius=spatial_radius, **opts)
    if filt and spatial_below is not None:
        filt.set_spatial(spatial_below, spatial_radius)
    with _on_device(frames, n * h * w * 12 if out_of_place else None, owned=None if filt else ff) as (d_frames, d_rgb):
        ff.run_frames(d_frames.ptr, n, samples, d_rgb=_ptr(d_rgb))
        f = d_frames.download(np.float32, frames.shape)
        return (f, d_rgb.download(np.float32, (n, h, w, 3))) if out_of_place else f


class TemporalOpts(ctypes.Structure):
    """pt_temporal_opts (include/ptcore.h)."""
    _fields_ = [("history_cap", ctypes.c_float), ("depth_tol", ctypes.c_float), ("normal_tol", ctypes.c_float),
                ("albedo_tol", ctypes.c_float), ("min_weight", ctypes.c_float), ("reserved", ctypes.c_int32)]


class TemporalAntilagOpts(ctypes.Structure):
    """pt_temporal_antilag_opts (include/ptcore.h)."""
    _fields_ = [("fast_cap", ctypes.c_float), ("clamp_sigma", ctypes.c_float), ("clamp_radius", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _antilag_defaults():
    o = TemporalAntilagOpts()
    lib.pt_temporal_antilag_opts_default(ctypes.byref(o))
    return {"fast_cap": float(o.fast_cap), "clamp_sigma": float(o.clamp_sigma), "clamp_radius": int(o.clamp_radius)}


ANTILAG_DEFAULTS = _antilag_defaults()  # pt_temporal_antilag_opts_default: fast_cap 0 (off), the library's clamp_sigma and clamp_radius


def temporal_antilag_check(fast_cap, clamp_sigma=ANTILAG_DEFAULTS["clamp_sigma"], clamp_radius=ANTILAG_DEFAULTS["clamp_radius"],
                           history_cap=256.0, reserved=0):
    """pt_temporal_antilag_check: the host checks of Temporal.set_antilag alone; host only.  Raises PtError for what it refuses."""
    opts = TemporalAntilagOpts(fast_cap=fast_cap, clamp_sigma=clamp_sigma, clamp_radius=clamp_radius, reserved=reserved)
    check(lib.pt_temporal_antilag_check(ctypes.byref(opts), history_cap))


def temporal_camera(basis):
    """pt_temporal_camera: the float32 inverse [3][3] of [B0 | B1-B0 | B2-B0] that carries a world offset from the eye to
    t (1, sy, v); host only.  Raises PtError for a degenerate or non-parallelogram basis."""
    _, b = _f32(basis, 12)
    out = np.zeros(9, dtype=np.float32)
    check(lib.pt_temporal_camera(b, out.ctypes.data_as(_fp)))
    return out.reshape(3, 3)


class Temporal(_Session):
    """ctypes view of pt_temporal: the temporal accumulator for width x height frames (DENOISER.md, "Temporal accumulation").
    Every call works in place on a device [H][W][14] frame of `samples` samples per pixel rendered with (basis, eye): channels
    0-2 and 10 become those of all the samples accumulated at the pixel's world position; d_counts, a device uint32 [H][W]
    image, receives the accumulated counts (FeatureFilter's d_counts)."""
    _destroy = "pt_temporal_destroy"

    def __init__(self, width, height, history_cap=256.0, depth_tol=0.02, normal_tol=0.9, albedo_tol=0.01, min_weight=0.25, fast_cap=0.0,
                 clamp_sigma=ANTILAG_DEFAULTS["clamp_sigma"], clamp_radius=ANTILAG_DEFAULTS["clamp_radius"]):
        opts = TemporalOpts(history_cap=history_cap, depth_tol=depth_tol, normal_tol=normal_tol, albedo_tol=albedo_tol, min_weight=min_weight)
        antilag = TemporalAntilagOpts(fast_cap=fast_cap, clamp_sigma=clamp_sigma, clamp_radius=clamp_radius)
        if fast_cap != 0.0:  # (refused here, before a session exists)
            check(lib.pt_temporal_antilag_check(ctypes.byref(antilag), history_cap))
        h = _vp()
        check(lib.pt_temporal_create(width, height, ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height = width, height
        if fast_cap != 0.0:
            self.set_antilag(fast_cap, clamp_sigma, clamp_radius)

    def set_antilag(self, fast_cap, clamp_sigma=ANTILAG_DEFAULTS["clamp_sigma"], clamp_radius=ANTILAG_DEFAULTS["clamp_radius"]):
        """pt_temporal_set_antilag: the responsive history (DENOISER.md, "Responsive history") on with fast_cap >= 1, off with 0.
        Only while the session holds no history: before its first frame or right after reset()."""
        opts = TemporalAntilagOpts(fast_cap=fast_cap, clamp_sigma=clamp_sigma, clamp_radius=clamp_radius)
        check(lib.pt_temporal_set_antilag(self.handle, ctypes.byref(opts)))

    def fast(self, out=None, stream=None):
        """pt_temporal_fast: the fast image the last call wrote, a float32 torch tensor [H][W][4] {fast rgb, fast count} on the
        current device (synchronous).  out: a tensor, a DeviceBuffer or a device address of width x height x 16 bytes to write
        into instead, asynchronously on `stream`, and to return."""
        if out is not None:
            check(lib.pt_temporal_fast(self.handle, self._device_ptr(out), stream))
            return out
        import torch

        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        check(lib.pt_temporal_fast(self.handle, out.data_ptr(), None))
        torch.cuda.synchronize()
        return out

    def memory(self):
        """{"workspace": bytes of the two history images (and, once a call with spheres= or scenes= needed it, of the session's
        motion image, and, once anti-lag was switched on, of the two fast images), "per_pixel": bytes per pixel: 96, + 16 with a
        motion image, + 32 with anti-lag}."""
        b = ctypes.c_uint64(0)
        check(lib.pt_temporal_workspace_bytes(self.handle, ctypes.byref(b)))
        return {"workspace": int(b.value), "per_pixel": int(b.value) // (self.width * self.height)}

    def reset(self):
        """Forget the history: the next frame passes through."""
        check(lib.pt_temporal_reset(self.handle))

    @staticmethod
    def _spheres(spheres):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
        return s, s.ctypes.data, len(s)

    @staticmethod
    def _device_ptr(image):
        """A device address from an int, a DeviceBuffer or a torch tensor."""
        return image.data_ptr() if hasattr(image, "data_ptr") else getattr(image, "ptr", image)

    def motion(self, spheres_now, spheres_prev, basis, eye=DEFAULT_EYE, out=None, stream=None):
        """pt_temporal_motion: the motion image of two index-matched host scenes under (basis, eye), a float32 torch tensor
        [H][W][4] {mx, my, mz, w} on the current device (synchronous).  Pass it as `motion=` to enqueue / run.
        out: a DeviceBuffer (or any device address) of width x height x 16 bytes to write into instead, asynchronously on
        `stream`, and to return: no torch is involved then."""
        now, pn, n = self._spheres(spheres_now)
        prev, pp, n_prev = self._spheres(spheres_prev)
        if n != n_prev:
            raise ValueError(f"motion: {n} spheres now, {n_prev} before: the scenes are index-matched")
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        if out is not None:
            check(lib.pt_temporal_motion(self.handle, pn, pp, n, b, e, self._device_ptr(out), stream))
            return out
        import torch

        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        check(lib.pt_temporal_motion(self.handle, pn, pp, n, b, e, out.data_ptr(), None))
        torch.cuda.synchronize()
        return out

    def enqueue(self, d_frame, samples, basis, eye=DEFAULT_EYE, d_counts=None, stream=None, motion=None, spheres=None):
        """motion: a device motion image [H][W][4] (self.motion, or any device address); spheres: the HOST scene the frame was
        rendered from (pt_temporal_enqueue_scene: the session remembers it and follows the spheres from call to call).  At most
        one of the two."""
        if motion is not None and spheres is not None:
            raise ValueError("motion and spheres are mutually exclusive")
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        if spheres is not None:
            _keep, ps, n = self._spheres(spheres)
            check(lib.pt_temporal_enqueue_scene(self.handle, d_frame, samples, b, e, ps, n, d_counts, stream))
        elif motion is not None:
            check(lib.pt_temporal_enqueue_motion(self.handle, d_frame, samples, b, e, self._device_ptr(motion), d_counts, stream))
        else:
            check(lib.pt_temporal_enqueue(self.handle, d_frame, samples, b, e, d_counts, stream))

    def run(self, d_frame, samples, basis, eye=DEFAULT_EYE, d_counts=None, motion=None, spheres=None):
        """Synchronous; returns device-event milliseconds.  motion, spheres: as for enqueue."""
        if motion is not None and spheres is not None:
            raise ValueError("motion and spheres are mutually exclusive")
        _, b = _f32(basis, 12)
        _, e = _f32(eye, 3)
        if spheres is not None:
            _keep, ps, n = self._spheres(spheres)
            return self._timed(lib.pt_temporal_run_scene, d_frame, samples, b, e, ps, n, d_counts)
        if motion is not None:
            return self._timed(lib.pt_temporal_run_motion, d_frame, samples, b, e, self._device_ptr(motion), d_counts)
        return self._timed(lib.pt_temporal_run, d_frame, samples, b, e, d_counts)

    def _scenes(self, scenes, n_frames):
        s = np.ascontiguousarray(scenes, dtype=SPHERE_DTYPE)
        if s.ndim != 2 or s.shape[0] != n_frames:
            raise ValueError(f"scenes: [{n_frames}][n] spheres expected, got shape {s.shape}")
        return s, s.ctypes.data, s.shape[1]

    def _cameras(self, bases, eyes, frame_stride_floats):
        bases = np.ascontiguousarray(bases, dtype=np.float32).reshape(-1, 12)
        eyes = np.ascontiguousarray(eyes, dtype=np.float32).reshape(-1, 3)
        assert len(bases) == len(eyes)
        fs = self.width * self.height * CHANNELS if frame_stride_floats is None else frame_stride_floats
        return bases, eyes, fs

    def enqueue_frames(self, d_frames, samples, bases, eyes, frame_stride_floats=None, d_counts=None, stream=None, scenes=None):
        """Asynchronous; the n = len(bases) frames at d_frames + k * frame_stride_floats (default: packed) in order, bit for
        bit n single enqueues; d_counts receives the last frame's counts.  scenes: host spheres [n][n_spheres], the scene of
        every frame (pt_temporal_enqueue_frames_scenes: bit for bit n single enqueues with spheres=)."""
        bases, eyes, fs = self._cameras(bases, eyes, frame_stride_floats)
        if scenes is not None:
            _keep, ps, n = self._scenes(scenes, len(bases))
            check(lib.pt_temporal_enqueue_frames_scenes(self.handle, len(bases), d_frames, fs, bases.ctypes.data_as(_fp),
                                                        eyes.ctypes.data_as(_fp), ps, n, samples, d_counts, stream))
            return
        check(lib.pt_temporal_enqueue_frames(self.handle, len(bases), d_frames, fs, bases.ctypes.data_as(_fp), eyes.ctypes.data_as(_fp),
                                             samples, d_counts, stream))

    def run_frames(self, d_frames, samples, bases, eyes, frame_stride_floats=None, d_counts=None, scenes=None):
        """Synchronous enqueue_frames; returns device-event milliseconds."""
        bases, eyes, fs = self._cameras(bases, eyes, frame_stride_floats)
        if scenes is not None:
            _keep, ps, n = self._scenes(scenes, len(bases))
            return self._timed(lib.pt_temporal_run_frames_scenes, len(bases), d_frames, fs, bases.ctypes.data_as(_fp),
                               eyes.ctypes.data_as(_fp), ps, n, samples, d_counts)
        return self._timed(lib.pt_temporal_run_frames, len(bases), d_frames, fs, bases.ctypes.data_as(_fp), eyes.ctypes.data_as(_fp),
                           samples, d_counts)


MOTION_CHUNK = 256  # PT_MOTION_CHUNK (include/ptcore.h): spheres per round of the motion kernel's staging


def temporal_scene_check(spheres_now, spheres_prev, basis, eye=DEFAULT_EYE):
    """pt_temporal_scene_check: the host checks of Temporal.motion alone; host only.  Raises PtError for what it refuses."""
    now = np.ascontiguousarray(spheres_now, dtype=SPHERE_DTYPE).reshape(-1)
    prev = np.ascontiguousarray(spheres_prev, dtype=SPHERE_DTYPE).reshape(-1)
    if len(now) != len(prev):
        raise ValueError("the scenes are index-matched")
    _, b = _f32(basis, 12)
    _, e = _f32(eye, 3)
    check(lib.pt_temporal_scene_check(now.ctypes.data, prev.ctypes.data, len(now), b, e))


def accumulate_frames(frames, samples, bases, eyes, temporal=None, scenes=None, **opts):
    """Convenience for tests, like filter_frames: host frames [N][H][W][14] of one fly-through through ONE
    pt_temporal_run_frames call of a fresh session (or `temporal`, whose history then goes in).  Returns (the frames after the
    stage, the uint32 [H][W] counts of the last frame).  scenes: host spheres [N][n], the scene of every frame (animated
    scenes: pt_temporal_run_frames_scenes).  opts: of the Temporal made here, fast_cap, clamp_sigma and clamp_radius (the
    responsive history) among them."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    n, h, w = frames.shape[:3]
    ta = temporal or Temporal(w, h, **opts)
    with _on_device(frames, h * w * 4, owned=None if temporal else ta) as (d_frames, d_counts):
        ta.run_frames(d_frames.ptr, samples, bases, eyes, d_counts=d_counts.ptr, scenes=scenes)
        return d_frames.download(np.float32, frames.shape), d_counts.download(np.uint32, (h, w))


TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
ENCODE_SRGB, ENCODE_LINEAR = 0, 1
TONEMAP_CURVES = {"clamp": TONEMAP_CLAMP, "reinhard": TONEMAP_REINHARD, "aces": TONEMAP_ACES}
TONEMAP_ENCODES = {"srgb": ENCODE_SRGB, "linear": ENCODE_LINEAR}


class TonemapOpts(ctypes.Structure):
    """pt_tonemap_opts (include/ptcore.h)."""
    _fields_ = [("curve", ctypes.c_int32), ("encode", ctypes.c_int32), ("exposure", ctypes.c_float), ("key", ctypes.c_float),
                ("white", ctypes.c_float), ("adapt", ctypes.c_float), ("max_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


def tonemap_srgb_table():
    """pt_tonemap_srgb_table: the 255 float32 thresholds of the sRGB codes 1 .. 255; host only."""
    out = np.zeros(255, dtype=np.float32)
    check(lib.pt_tonemap_srgb_table(out.ctypes.data_as(_fp)))
    return out


class Tonemap(_BatchedStage):
    """ctypes view of pt_tonemap: the tone-mapping session for width x height images (DENOISER.md, "Tone mapping").  A call reads
    a device image of linear radiance [H][W][pixel_stride] (14: a frame, 3: a filter's or denoiser's d_rgb; never written) and
    writes device RGBA8 uint32 [H][W].  curve: "clamp" | "reinhard" | "aces"; encode: "srgb" | "linear"; exposure: "auto"
    (metered on the device and adapted from frame to frame at rate `adapt`) or a number > 0."""
    _destroy, _reserve = "pt_tonemap_destroy", "pt_tonemap_reserve_frames"

    def __init__(self, width, height, curve="aces", encode="srgb", exposure="auto", key=0.18, white=4.0, adapt=1.0, max_frames=1):
        if curve not in TONEMAP_CURVES:
            raise ValueError(f"curve {curve!r}: one of {sorted(TONEMAP_CURVES)}")
        if encode not in TONEMAP_ENCODES:
            raise ValueError(f"encode {encode!r}: one of {sorted(TONEMAP_ENCODES)}")
        if exposure != "auto" and float(exposure) == 0.0:
            raise ValueError("exposure 0: 'auto' or a number > 0")
        opts = TonemapOpts(curve=TONEMAP_CURVES[curve], encode=TONEMAP_ENCODES[encode], exposure=0.0 if exposure == "auto" else float(exposure),
                           key=key, white=white, adapt=adapt, max_frames=max_frames)
        h = _vp()
        check(lib.pt_tonemap_create(width, height, ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height = width, height
        self.max_frames = max_frames

    def memory(self):
        """{"workspace": bytes of the table, the state and the partial sums of all max_frames frames}."""
        b = ctypes.c_uint64(0)
        check(lib.pt_tonemap_workspace_bytes(self.handle, ctypes.byref(b)))
        return {"workspace": int(b.value)}

    def reset(self):
        """Forget the exposure: the next frame's exposure is its own target."""
        check(lib.pt_tonemap_reset(self.handle))

    def exposure(self):
        """Synchronous: the exposure of the last frame (float32)."""
        e = ctypes.c_float(0)
        check(lib.pt_tonemap_exposure(self.handle, ctypes.byref(e)))
        return np.float32(e.value)

    def enqueue(self, d_src, d_rgba8, pixel_stride=CHANNELS, stream=None):
        check(lib.pt_tonemap_enqueue(self.handle, d_src, pixel_stride, d_rgba8, stream))

    def run(self, d_src, d_rgba8, pixel_stride=CHANNELS):
        """Synchronous; returns device-event milliseconds."""
        return self._timed(lib.pt_tonemap_run, d_src, pixel_stride, d_rgba8)

    def enqueue_frames(self, d_src, n, d_rgba8, pixel_stride=CHANNELS, src_stride_floats=None, dst_stride_pixels=None, stream=None):
        """Asynchronous; n images at d_src + k * src_stride_floats (default: packed) to d_rgba8 + k * dst_stride_pixels, in order:
        bit for bit n single enqueues, the adaptation included."""
        ss, ds = self._strides(src_stride_floats, dst_stride_pixels, pixel_stride, 1)
        check(lib.pt_tonemap_enqueue_frames(self.handle, n, d_src, ss, pixel_stride, d_rgba8, ds, stream))

    def run_frames(self, d_src, n, d_rgba8, pixel_stride=CHANNELS, src_stride_floats=None, dst_stride_pixels=None):
        """Synchronous enqueue_frames; returns device-event milliseconds."""
        ss, ds = self._strides(src_stride_floats, dst_stride_pixels, pixel_stride, 1)
        return self._timed(lib.pt_tonemap_run_frames, n, d_src, ss, pixel_stride, d_rgba8, ds)


def tonemap_frame(frame_or_rgb, tonemap=None, **opts):
    """Convenience for tests: upload a host [H][W][C] image (C = 14: a frame, 3: an rgb image, anything in 3 .. 64), tone-map it
    on the GPU, download.  Returns uint8 [H][W][4].  opts: of the Tonemap made here (curve, encode, exposure, ...)."""
    img = np.ascontiguousarray(frame_or_rgb, dtype=np.float32)
    h, w, c = img.shape
    tm = tonemap or Tonemap(w, h, **opts)
    with _on_device(img, h * w * 4, owned=None if tonemap else tm) as (d_src, d_out):
        tm.run(d_src.ptr, d_out.ptr, pixel_stride=c)
        return d_out.download(np.uint8, (h, w, 4))


# ---- frame comparison -----------------------------------------------------------------
class CompareOpts(ctypes.Structure):
    """pt_compare_opts (include/ptcore.h)."""
    _fields_ = [("max_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class CompareValues(ctypes.Structure):
    """pt_compare_values (include/ptcore.h)."""
    _fields_ = [("sum_mse", ctypes.c_uint64), ("sum_relmse", ctypes.c_uint64), ("sum_ssim", ctypes.c_int64), ("pixels", ctypes.c_uint64),
                ("saturated", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64), ("mse", ctypes.c_double), ("rms", ctypes.c_double),
                ("psnr", ctypes.c_double), ("relmse", ctypes.c_double), ("ssim", ctypes.c_double)]


def ssim_weights():
    """pt_compare_ssim_weights: the eleven float32 weights of the SSIM window; host only."""
    out = np.zeros(11, dtype=np.float32)
    check(lib.pt_compare_ssim_weights(out.ctypes.data_as(_fp)))
    return out


class Compare(_BatchedStage):
    """ctypes view of pt_compare: the comparison session for width x height images (DENOISER.md, "Frame comparison").  A call
    reads two device images [H][W][pixel_stride] (14: a frame, 3: an rgb image; the two strides are independent), writes neither
    and leaves clamped MSE, relMSE and SSIM of each frame on the device; d_map (optional) receives [H][W][3] = (m, r, s)."""
    _destroy, _reserve = "pt_compare_destroy", "pt_compare_reserve_frames"

    def __init__(self, width, height, max_frames=1):
        opts = CompareOpts(max_frames=max_frames)
        h = _vp()
        check(lib.pt_compare_create(width, height, ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height = width, height
        self.max_frames = max_frames

    def memory(self):
        """{"workspace": bytes of the partial sums of all max_frames frames and of the records}."""
        b = ctypes.c_uint64(0)
        check(lib.pt_compare_workspace_bytes(self.handle, ctypes.byref(b)))
        return {"workspace": int(b.value)}

    def enqueue(self, d_img, d_ref, d_map=None, img_pixel_stride=CHANNELS, ref_pixel_stride=CHANNELS, stream=None):
        check(lib.pt_compare_enqueue(self.handle, d_img, img_pixel_stride, d_ref, ref_pixel_stride, d_map, stream))

    def run(self, d_img, d_ref, d_map=None, img_pixel_stride=CHANNELS, ref_pixel_stride=CHANNELS):
        """Synchronous; returns device-event milliseconds."""
        return self._timed(lib.pt_compare_run, d_img, img_pixel_stride, d_ref, ref_pixel_stride, d_map)

    def _frame_strides(self, img_px, ref_px, img_stride, ref_stride, map_stride):
        px = self.width * self.height
        return (px * img_px if img_stride is None else img_stride, px * ref_px if ref_stride is None else ref_stride,
                px * 3 if map_stride is None else map_stride)

    def enqueue_frames(self, d_img, n, d_ref, d_map=None, img_pixel_stride=CHANNELS, ref_pixel_stride=CHANNELS, img_stride_floats=None,
                       ref_stride_floats=None, map_stride_floats=None, stream=None):
        """Asynchronous; frame k compares d_img + k * img_stride_floats with d_ref + k * ref_stride_floats (default: packed;
        ref_stride_floats=0: one reference for all n frames): bit for bit n single enqueues."""
        si, sr, sm = self._frame_strides(img_pixel_stride, ref_pixel_stride, img_stride_floats, ref_stride_floats, map_stride_floats)
        check(lib.pt_compare_enqueue_frames(self.handle, n, d_img, si, img_pixel_stride, d_ref, sr, ref_pixel_stride, d_map, sm, stream))

    def run_frames(self, d_img, n, d_ref, d_map=None, img_pixel_stride=CHANNELS, ref_pixel_stride=CHANNELS, img_stride_floats=None,
                   ref_stride_floats=None, map_stride_floats=None):
        """Synchronous enqueue_frames; returns device-event milliseconds."""
        si, sr, sm = self._frame_strides(img_pixel_stride, ref_pixel_stride, img_stride_floats, ref_stride_floats, map_stride_floats)
        return self._timed(lib.pt_compare_run_frames, n, d_img, si, img_pixel_stride, d_ref, sr, ref_pixel_stride, d_map, sm)

    def result(self, k=0):
        """Synchronous: frame k of the last call as a dict -- the integer sums (sum_mse, sum_relmse, sum_ssim), pixels, saturated,
        nonfinite, and the doubles mse, rms, psnr, relmse, ssim."""
        v = CompareValues()
        check(lib.pt_compare_result(self.handle, k, ctypes.byref(v)))
        return {name: getattr(v, name) for name, _ in CompareValues._fields_}

    def results(self, n):
        return [self.result(k) for k in range(n)]


def compare_frames(img, ref, want_map=False, compare=None):
    """Convenience for tests: upload two host images [H][W][C] (C = 14: a frame, 3: an rgb image, anything in 3 .. 64; the two may
    differ in C), compare them on the GPU.  Returns the result dict, and the [H][W][3] map (m, r, s) too when want_map."""
    img, ref = np.ascontiguousarray(img, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    h, w, c = img.shape
    if ref.shape[:2] != (h, w):
        raise ValueError(f"compare_frames: image {w} x {h}, reference {ref.shape[1]} x {ref.shape[0]}")
    cmp_ = compare or Compare(w, h)
    with _on_device(img, ref, h * w * 12 if want_map else None, owned=None if compare else cmp_) as (d_img, d_ref, d_map):
        cmp_.run(d_img.ptr, d_ref.ptr, _ptr(d_map), img_pixel_stride=c, ref_pixel_stride=ref.shape[2])
        res = cmp_.result(0)
        return (res, d_map.download(np.float32, (h, w, 3))) if want_map else res


# ---- training patches -----------------------------------------------------------------
class PatchesOpts(ctypes.Structure):
    """pt_patches_opts (include/ptcore.h)."""
    _fields_ = [("patch", ctypes.c_int32), ("max_patches", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class PatchesValues(ctypes.Structure):
    """pt_patches_values (include/ptcore.h)."""
    _fields_ = [("colour_s1", ctypes.c_int64), ("colour_a", ctypes.c_uint64), ("colour_b", ctypes.c_uint64), ("colour_c", ctypes.c_uint64),
                ("normal_s1", ctypes.c_int64), ("normal_a", ctypes.c_uint64), ("normal_b", ctypes.c_uint64), ("normal_c", ctypes.c_uint64),
                ("values", ctypes.c_uint64), ("var_colour", ctypes.c_double), ("var_normal", ctypes.c_double), ("score", ctypes.c_double)]


def _corner_array(corners):
    """Corners as the C ABI takes them: a contiguous int32 [n][2] host array of (x, y)."""
    a = np.asarray(corners, dtype=np.int64).reshape(-1, 2)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("a corner does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


class Patches(_Session):
    """ctypes view of pt_patches: the training-patch session for width x height frames, patches of `patch` x `patch` pixels, up
    to max_patches per call (DENOISER.md, "Training patches").  prepare(d_train) meters the frame's divisors; score and gather take
    the same device [H][W][14] frame again with host corners [(x, y), ...] and write neither it nor the target image."""
    _destroy = "pt_patches_destroy"

    def __init__(self, width, height, patch, max_patches=64):
        opts = PatchesOpts(patch=patch, max_patches=max_patches)
        h = _vp()
        check(lib.pt_patches_create(width, height, ctypes.byref(opts), ctypes.byref(h)))
        self.handle = h.value
        self.width, self.height, self.patch, self.max_patches = width, height, patch, max_patches

    def memory(self):
        """{"workspace": device bytes of the maxima, the corners, the partial sums and the records}."""
        b = ctypes.c_uint64(0)
        check(lib.pt_patches_workspace_bytes(self.handle, ctypes.byref(b)))
        return {"workspace": int(b.value)}

    def prepare(self, d_train, stream=None):
        """Asynchronous: the divisors of this frame; needed again for every new frame."""
        check(lib.pt_patches_prepare(self.handle, d_train, stream))

    def run_prepare(self, d_train):
        """Synchronous prepare; returns device-event milliseconds."""
        return self._timed(lib.pt_patches_run_prepare, d_train)

    def enqueue_score(self, d_train, corners, stream=None):
        c = _corner_array(corners)
        check(lib.pt_patches_score(self.handle, d_train, len(c), c.ctypes.data, stream))

    def score(self, d_train, corners):
        """Synchronous enqueue_score; returns device-event milliseconds (the values: result / results)."""
        c = _corner_array(corners)
        return self._timed(lib.pt_patches_run_score, d_train, len(c), c.ctypes.data)

    def result(self, k=0):
        """Synchronous: patch k of the last score call as a dict -- the eight integer sums, values, and the doubles var_colour,
        var_normal, score."""
        v = PatchesValues()
        check(lib.pt_patches_result(self.handle, k, ctypes.byref(v)))
        return {name: getattr(v, name) for name, _ in PatchesValues._fields_}

    def results(self, n):
        return [self.result(k) for k in range(n)]

    def enqueue_gather(self, d_train, corners, d_inputs, d_gt=None, d_targets=None, gt_pixel_stride=CHANNELS, stream=None):
        """Asynchronous: d_inputs receives [n][14][P][P] floats, d_targets (optional, from the device image d_gt) [n][3][P][P]."""
        c = _corner_array(corners)
        check(lib.pt_patches_gather(self.handle, d_train, d_gt, gt_pixel_stride, len(c), c.ctypes.data, d_inputs, d_targets, stream))

    def gather(self, d_train, corners, d_inputs, d_gt=None, d_targets=None, gt_pixel_stride=CHANNELS):
        """Synchronous enqueue_gather; returns device-event milliseconds."""
        c = _corner_array(corners)
        return self._timed(lib.pt_patches_run_gather, d_train, d_gt, gt_pixel_stride, len(c), c.ctypes.data, d_inputs, d_targets)


def pick_patches(scores, n, rng):
    """The reference's selection among scored candidates (load_data.py: get_patches): the total of the scores is fixed once;
    the remaining candidates are scanned in order, each taken with probability score / total -- or unconditionally once more
    than 10 n candidates have been passed over; a take removes the candidate and restarts the scan, until n are taken.  rng is a
    random.Random (one random() per candidate looked at).  A total of 0 makes every probability 0, where the reference would
    divide by zero.  Returns the n indices into `scores`, in the order taken."""
    scores = [float(s) for s in scores]
    if n > len(scores):
        raise ValueError(f"pick_patches: n = {n} of {len(scores)} candidates")
    total = 0.0
    for s in scores:
        total += s
    left, picked, passed = list(range(len(scores))), [], 0
    while len(picked) < n:
        for pos, k in enumerate(left):
            p = scores[k] / total if total != 0.0 else 0.0
            if rng.random() < p or passed > 10 * n:
                picked.append(k)
                del left[pos]
                break
            passed += 1
    return picked


def training_patches(train, gt, patch_size=256, num_patches=16, rng=None, patches=None):
    """The reference's get_patches on the device: from a host train frame [H][W][14] and a host target image [H][W][C] (C in
    3 .. 64, colour first), draw 4 num_patches corners with rng (a random.Random; x then y, each from the reference's range
    randint(0, side - patch_size - 1)), score them on the GPU, pick num_patches with pick_patches and gather those.  Returns
    (inputs [N][14][P][P], targets [N][3][P][P], corners int32 [N][2] as (x, y), scores float64 [N]) of the picked patches.
    patches: a Patches session of this frame size and patch_size with max_patches >= 4 num_patches, instead of one made here."""
    import random

    train, gt = np.ascontiguousarray(train, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
    h, w, c = train.shape
    if c != CHANNELS or gt.shape[:2] != (h, w):
        raise ValueError(f"training_patches: train {train.shape}, target {gt.shape}: [H][W][14] and [H][W][C] of one size")
    rng = rng or random.Random()
    p, n, cand = patch_size, num_patches, 4 * num_patches
    ps = patches or Patches(w, h, p, max_patches=cand)
    if (ps.width, ps.height, ps.patch) != (w, h, p) or ps.max_patches < cand:
        raise ValueError(f"training_patches: the session is for {ps.width} x {ps.height}, patch {ps.patch}, {ps.max_patches} patches")
    corners = [(rng.randint(0, max(w - p - 1, 0)), rng.randint(0, max(h - p - 1, 0))) for _ in range(cand)]
    with _on_device(train, gt, n * 14 * p * p * 4, n * 3 * p * p * 4, owned=None if patches else ps) as (d_train, d_gt, d_in, d_out):
        ps.prepare(d_train.ptr)
        ps.score(d_train.ptr, corners)
        scores = [r["score"] for r in ps.results(cand)]
        picked = pick_patches(scores, n, rng)
        chosen = _corner_array([corners[k] for k in picked])
        ps.gather(d_train.ptr, chosen, d_in.ptr, d_gt=d_gt.ptr, d_targets=d_out.ptr, gt_pixel_stride=gt.shape[2])
        return (d_in.download(np.float32, (n, 14, p, p)), d_out.download(np.float32, (n, 3, p, p)), chosen,
                np.array([scores[k] for k in picked], dtype=np.float64))
