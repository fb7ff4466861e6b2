// pt_debug.hip -- LAB LIBRARY ONLY (libptcore_lab.so, include/ptcore_lab.h): diagnostic entry points that evaluate the
// device-side scalar building blocks elementwise, and compare two of them over a range of
// float bit patterns.  Used by the tests to (1) check the device definitions of sin/cos,
// sqrt, 1/sqrt against the CPU oracle on dense samples and (2) PROVE by exhaustion that the
// cheap sequences of pt_device.h equal the literal expressions for every float.
#include "pt_device.h"
#include "pt_internal.h"
#include "pt_kernel.h"
#include "../../include/ptcore_lab.h"

#pragma clang fp contract(off)

namespace pt {

__device__ __forceinline__ float eval_unary(int fn, float x) {
  float s, c;
  switch (fn) {
    case PT_FN_INV_SQRT_LITERAL: return 1.0f / sqrtf(x);
    case PT_FN_INV_SQRT_FAST: return inv_sqrt_spec(x);
    case PT_FN_SQRT_LITERAL: return sqrtf(x);
    case PT_FN_SQRT_FAST: return sqrt_cr_f32(x);
    case PT_FN_SIN: pt_sincos(x, s, c); return s;
    case PT_FN_COS: pt_sincos(x, s, c); return c;
    case PT_FN_UNIFORM: return uniform_from_u32(__float_as_uint(x));
    case PT_FN_ONEMINUS_LITERAL: return (float)sqrt(1.0 - (double)(x * x));
    case PT_FN_ONEMINUS_FAST: return (float)sqrt_cr(1.0 - (double)(x * x));
    case PT_FN_ONEMINUS_F32: {
      bool bad = false;
      const float v = oneminus_f32_nb(x, bad);
      return bad ? (float)sqrt(1.0 - (double)(x * x)) : v;
    }
    case PT_FN_ONEMINUS_F32_FLAG: {
      bool bad = false;
      (void)oneminus_f32_nb(x, bad);
      return bad ? 1.0f : 0.0f;
    }
    case PT_FN_ZERO: return 0.0f;
    case PT_FN_UNIFORM_LITERAL: return uniform_from_u32_literal(__float_as_uint(x));
    case PT_FN_SIN_LITERAL: pt_sincos_literal(x, s, c); return s;
    case PT_FN_COS_LITERAL: pt_sincos_literal(x, s, c); return c;
    default: return __builtin_nanf("");
  }
}

__global__ void __launch_bounds__(256) unary_map_kernel(int fn, const float* in, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = eval_unary(fn, in[i]);
}

// result[0] = number of bit patterns where fn_a != fn_b (NaN == NaN), result[1] = one such pattern
__global__ void __launch_bounds__(256) unary_compare_kernel(int fn_a, int fn_b, uint32_t first, uint64_t count,
                                                            unsigned long long* result) {
  unsigned long long bad = 0, example = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
    const uint32_t bits = first + (uint32_t)i;
    const float x = __uint_as_float(bits);
    const float a = eval_unary(fn_a, x), b = eval_unary(fn_b, x);
    const bool same = (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b);
    if (!same) {
      bad++;
      example = bits;
    }
  }
  if (bad) {
    atomicAdd(&result[0], bad);
    atomicExch(&result[1], example);
  }
}

// the kernels' division by a sample count against the division: result[0] = mismatches, [1] = dividend bits, [2] = count
__global__ void __launch_bounds__(256) div_compare_kernel(uint32_t n_first, uint32_t n_count, uint32_t first, uint64_t count,
                                                          unsigned long long* result) {
  unsigned long long bad = 0, ex_bits = 0, ex_n = 0;
  for (uint32_t k = 0; k < n_count; k++) {
    const uint32_t n = n_first + k;
    const float nf = (float)n;
    const float y = (n <= (uint32_t)kRcpTab) ? 1.0f / nf : __builtin_nanf("");  // what SceneLds::rcpn holds for this count
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
      const uint32_t bits = first + (uint32_t)i;
      const float delta = __uint_as_float(bits);
      const float a = div_by_count(delta, nf, y), b = delta / nf;
      const bool same = (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b);
      if (!same) {
        bad++;
        ex_bits = bits;
        ex_n = n;
      }
    }
  }
  if (bad) {
    atomicAdd(&result[0], bad);
    atomicExch(&result[1], ex_bits);
    atomicExch(&result[2], ex_n);
  }
}

}  // namespace pt

extern "C" int pt_debug_unary_map(int fn, const float* d_in, float* d_out, size_t n) {
  if (fn < 0 || fn >= PT_FN_COUNT || (n && (!d_in || !d_out))) return pt_fail(PT_EINVAL, "pt_debug_unary_map: bad arguments");
  if (!n) return PT_OK;
  const unsigned grid = (unsigned)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536);
  hipLaunchKernelGGL(pt::unary_map_kernel, dim3(grid), dim3(256), 0, 0, fn, d_in, d_out, n);
  PT_HIPD(hipGetLastError());
  PT_HIPD(hipDeviceSynchronize());
  return PT_OK;
}

extern "C" int pt_debug_unary_compare(int fn_a, int fn_b, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch,
                                      uint32_t* example_bits) {
  if (fn_a < 0 || fn_a >= PT_FN_COUNT || fn_b < 0 || fn_b >= PT_FN_COUNT || !n_mismatch || count > (1ull << 32))
    return pt_fail(PT_EINVAL, "pt_debug_unary_compare: bad arguments");
  unsigned long long* d = nullptr;
  PT_HIPD(hipMalloc((void**)&d, 16));
  PT_HIPD(hipMemset(d, 0, 16));
  hipLaunchKernelGGL(pt::unary_compare_kernel, dim3(16384), dim3(256), 0, 0, fn_a, fn_b, first_bits, count, d);
  hipError_t e = hipGetLastError();
  unsigned long long h[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, d, 16, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return pt_fail(PT_EHIP, "pt_debug_unary_compare: %s", hipGetErrorString(e));
  *n_mismatch = h[0];
  if (example_bits) *example_bits = (uint32_t)h[1];
  return PT_OK;
}

extern "C" int pt_debug_div_compare(uint32_t n_first, uint32_t n_count, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch,
                                    uint32_t* example_bits, uint32_t* example_n) {
  if (!n_mismatch || count > (1ull << 32) || n_first < 1 || n_count < 1 || n_count > 4096)
    return pt_fail(PT_EINVAL, "pt_debug_div_compare: bad arguments");
  unsigned long long* d = nullptr;
  PT_HIPD(hipMalloc((void**)&d, 24));
  PT_HIPD(hipMemset(d, 0, 24));
  hipLaunchKernelGGL(pt::div_compare_kernel, dim3(16384), dim3(256), 0, 0, n_first, n_count, first_bits, count, d);
  hipError_t e = hipGetLastError();
  unsigned long long h[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return pt_fail(PT_EHIP, "pt_debug_div_compare: %s", hipGetErrorString(e));
  *n_mismatch = h[0];
  if (example_bits) *example_bits = (uint32_t)h[1];
  if (example_n) *example_n = (uint32_t)h[2];
  return PT_OK;
}

// diagnostics: build variant 11's grid for a scene and return its 16-word header
extern "C" int pt_debug_grid_header(const pt_sphere* d_spheres, int n_spheres, uint32_t header_out[16]) {
  if (!d_spheres || !header_out || n_spheres < 1) return pt_fail(PT_EINVAL, "pt_debug_grid_header: bad arguments");
  uint32_t* d = nullptr;
  PT_HIPD(hipMalloc((void**)&d, pt_kernel_accel_bytes()));
  hipError_t e = pt_launch_build_grid(d_spheres, n_spheres, d, nullptr, true, nullptr);
  if (e == hipSuccess) e = hipMemcpy(header_out, d, 64, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  PT_HIPD(e);
  return PT_OK;
}

// diagnostics: the whole accelerator image build_grid_kernel writes for a scene (header, out-of-grid list, cell starts, registrations,
// the pooled walk's cell table, emission data) and the byte offsets of its parts -- tests/test_grid_builder_gpu.py checks the
// registrations against the geometry in float64
extern "C" int pt_debug_grid_image(const pt_sphere* d_spheres, int n_spheres, const float* eye, int threads, uint32_t* image_out,
                                   size_t image_bytes, uint64_t layout_out[8]) {
  if (!d_spheres || !layout_out || n_spheres < 1) return pt_fail(PT_EINVAL, "pt_debug_grid_image: bad arguments");
  pt_kernel_grid_layout(n_spheres, threads, layout_out);
  const size_t need = (size_t)layout_out[0];
  if (!image_out) return PT_OK;  // (size query)
  if (image_bytes < need) return pt_fail(PT_EINVAL, "pt_debug_grid_image: the image needs %zu bytes", need);
  uint32_t* d = nullptr;
  PT_HIPD(hipMalloc((void**)&d, need));
  hipError_t e = hipMemset(d, 0, need);
  if (e == hipSuccess) e = pt_launch_build_grid(d_spheres, n_spheres, d, eye, true, nullptr, threads);
  if (e == hipSuccess) e = hipMemcpy(image_out, d, need, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  PT_HIPD(e);
  return PT_OK;
}

#if PT_BUILD_EXPERIMENTS
// ---- the two primary-ray exclusion analyses on their own (include/ptcore_lab.h; the kernels: pt_kernel.hip's lab section) --------
static bool primary_dump_args(PrimaryDumpArgs& a, const pt_sphere* d_spheres, int n, const float* eye, const float* basis, int width,
                              int height, int row_begin, int row_end) {
  if (!d_spheres || !eye || !basis || n < 1 || width < 1 || height < 1 || width > 16384 || height > 16384 || row_begin < 0 ||
      row_end <= row_begin || row_end > height)
    return false;
  a.spheres = d_spheres;
  a.n_spheres = n;
  for (int k = 0; k < 3; k++) a.eye[k] = eye[k];
  for (int k = 0; k < 12; k++) a.basis[k] = basis[k];
  a.width = width;
  a.height = height;
  a.row_begin = row_begin;
  a.tile_pixels = (uint32_t)(row_end - row_begin) * (uint32_t)width;
  return true;
}

extern "C" int pt_debug_primary_masks(const pt_sphere* d_spheres, int n_spheres, const float eye[3], const float basis[12], int width,
                                      int height, int row_begin, int row_end, uint32_t* d_masks, float* d_dirs) {
  PrimaryDumpArgs a;
  if (!d_masks || n_spheres > 64 || !primary_dump_args(a, d_spheres, n_spheres, eye, basis, width, height, row_begin, row_end))
    return pt_fail(PT_EINVAL, "pt_debug_primary_masks: bad arguments (1 .. 64 spheres, rows inside the image)");
  PT_HIPD(pt_launch_primary_masks_dump(a, d_masks, d_dirs));
  PT_HIPD(hipDeviceSynchronize());
  return PT_OK;
}

extern "C" int pt_debug_primary_lists(const pt_sphere* d_spheres, int n_spheres, const float eye[3], const float basis[12], int width,
                                      int height, int row_begin, int row_end, int threads, uint32_t* d_lists, uint32_t header_out[20]) {
  PrimaryDumpArgs a;
  if (!d_lists || !header_out || (threads != PT_GRID_BLOCK_THREADS && threads != PT_GRID_WIDE_THREADS) ||
      !primary_dump_args(a, d_spheres, n_spheres, eye, basis, width, height, row_begin, row_end))
    return pt_fail(PT_EINVAL, "pt_debug_primary_lists: bad arguments (threads 512 or 1024, rows inside the image)");
  uint32_t* d = nullptr;  // the grid exactly as pt_debug_grid_image builds it
  PT_HIPD(hipMalloc((void**)&d, pt_kernel_accel_bytes()));
  hipError_t e = hipMemset(d, 0, pt_kernel_accel_bytes());
  if (e == hipSuccess) e = pt_launch_build_grid(d_spheres, n_spheres, d, eye, true, nullptr, threads);
  if (e == hipSuccess) e = hipMemcpy(header_out, d, 20 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && header_out[0] != 0u) {  // (an invalid grid is reported in the header: nothing is launched, no list is written)
    e = pt_launch_primary_lists_dump(a, d, threads, d_lists);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  (void)hipFree(d);
  PT_HIPD(e);
  return PT_OK;
}

// ---- the adaptive selection and finalize kernels on states the caller builds (include/ptcore_lab.h) ----------------------------
// Host code only: the launchers are pt_adaptive.hip's own.  Every device array is an allocation of its own, filled with a sentinel
// before the caller's data goes over its front, and followed by 64 guard words; a guard that changed is reported by name.
namespace {

constexpr size_t kGuardBytes = 256;  // 64 words (the mask: 256 bytes)
constexpr int kSentinel = 0xA5;

struct GuardedArray {
  const char* name = "";
  uint8_t* d = nullptr;
  size_t bytes = 0;
  ~GuardedArray() {
    if (d) (void)hipFree(d);
  }
  hipError_t create(const char* nm, const void* host, size_t n) {
    name = nm;
    bytes = n;
    hipError_t e = hipMalloc((void**)&d, n + kGuardBytes);
    if (e == hipSuccess) e = hipMemset(d, kSentinel, n + kGuardBytes);
    if (e == hipSuccess && host && n) e = hipMemcpy(d, host, n, hipMemcpyHostToDevice);
    return e;
  }
  // the array back to the host (host may be NULL) and the guard read: *broken = the first array whose guard changed
  hipError_t finish(void* host, const char** broken) {
    uint8_t g[kGuardBytes];
    hipError_t e = (host && bytes) ? hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(g, d + bytes, kGuardBytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < kGuardBytes; i++)
      if (g[i] != (uint8_t)kSentinel && !*broken) *broken = name;
    return hipSuccess;
  }
};

}  // namespace

extern "C" int pt_debug_adaptive_select(const uint32_t* rec, uint32_t tile_pixels, int width, int n, int n_end, int mode, int peek,
                                        const pt_adaptive_opts* opts, uint8_t* mask, uint32_t* counts, uint32_t* list,
                                        uint32_t words[2], uint32_t* block_sums) {
  if (!rec || !opts || !mask || !counts || !list || !words || !tile_pixels)
    return pt_fail(PT_EINVAL, "pt_debug_adaptive_select: NULL argument or an empty tile");
  if (opts->radius < 0 || opts->radius > PT_ADAPTIVE_MAX_RADIUS)
    return pt_fail(PT_EINVAL, "pt_debug_adaptive_select: radius %d (0..%d)", opts->radius, PT_ADAPTIVE_MAX_RADIUS);
  const size_t tp = tile_pixels, n_blocks = (tp + PT_ADAPTIVE_BLOCK - 1) / PT_ADAPTIVE_BLOCK;
  GuardedArray g_rec, g_mask, g_counts, g_list, g_words, g_sums;
  PT_HIPD(g_rec.create("rec", rec, (size_t)PT_CHUNK_WORDS * tp * sizeof(uint32_t)));
  PT_HIPD(g_mask.create("mask", mask, tp));
  PT_HIPD(g_counts.create("counts", counts, tp * sizeof(uint32_t)));
  PT_HIPD(g_list.create("list", list, tp * sizeof(uint32_t)));
  PT_HIPD(g_words.create("words", words, 2 * sizeof(uint32_t)));
  PT_HIPD(g_sums.create("block_sums", nullptr, n_blocks * sizeof(uint32_t)));
  AdaptiveState s{};
  s.counts = (uint32_t*)g_counts.d;
  s.list = (uint32_t*)g_list.d;
  s.mask = g_mask.d;
  s.block_sums = (uint32_t*)g_sums.d;
  s.words = (uint32_t*)g_words.d;
  const AdaptiveRule rule = pt_adaptive_rule(*opts);
  const hipError_t e = pt_launch_adaptive_select(s, rule, (const uint32_t*)g_rec.d, tile_pixels, width, n, n_end, mode, peek != 0, nullptr);
  if (e == hipErrorInvalidValue) return pt_fail(PT_EINVAL, "pt_debug_adaptive_select: the launcher refused the arguments");
  PT_HIPD(e);
  PT_HIPD(hipDeviceSynchronize());
  const char* broken = nullptr;
  PT_HIPD(g_rec.finish(nullptr, &broken));
  PT_HIPD(g_mask.finish(mask, &broken));
  PT_HIPD(g_counts.finish(counts, &broken));
  PT_HIPD(g_list.finish(list, &broken));
  PT_HIPD(g_words.finish(words, &broken));
  PT_HIPD(g_sums.finish(block_sums, &broken));
  if (broken) return pt_fail(PT_EHIP, "pt_debug_adaptive_select: the guard words behind %s were written", broken);
  return PT_OK;
}

extern "C" int pt_debug_adaptive_finalize(const uint32_t* rec, const uint32_t* counts, uint32_t tile_pixels, int planar, float* out) {
  if (!rec || !counts || !out || !tile_pixels) return pt_fail(PT_EINVAL, "pt_debug_adaptive_finalize: NULL argument or an empty tile");
  const size_t tp = tile_pixels;
  GuardedArray g_rec, g_counts, g_out;
  PT_HIPD(g_rec.create("rec", rec, (size_t)PT_CHUNK_WORDS * tp * sizeof(uint32_t)));
  PT_HIPD(g_counts.create("counts", counts, tp * sizeof(uint32_t)));
  PT_HIPD(g_out.create("out", nullptr, tp * 14 * sizeof(float)));
  PT_HIPD(pt_launch_adaptive_finalize((const uint32_t*)g_rec.d, (const uint32_t*)g_counts.d, (float*)g_out.d, tile_pixels, planar != 0, nullptr));
  PT_HIPD(hipDeviceSynchronize());
  const char* broken = nullptr;
  PT_HIPD(g_rec.finish(nullptr, &broken));
  PT_HIPD(g_counts.finish(nullptr, &broken));
  PT_HIPD(g_out.finish(out, &broken));
  if (broken) return pt_fail(PT_EHIP, "pt_debug_adaptive_finalize: the guard words behind %s were written", broken);
  return PT_OK;
}
#endif
