// pt_tonemap.hip -- the tone-mapping session behind pt_tonemap_* (include/ptcore.h): the stage between a frame of linear
// radiance and a picture.  A metered exposure (the integer mean of the luminances' float bit patterns: a geometric mean whose sum
// is exact in any order), eye adaptation from frame to frame, a tone curve (clamp, luminance Reinhard, Narkowicz's ACES fit) and
// the correctly rounded 8-bit sRGB encode by table search.  No counterpart in the reference, whose display path is
// pt_display.hip's clamp.  DENOISER.md, "Tone mapping", states the definition; tests/tonemap_model.py restates it in NumPy.
// EXACT code, like pt_temporal.hip: no contraction, IEEE divisions, no transcendental on the device -- the kernels are held to
// the float32 model bit for bit.
//
// Three kernels, one lane per pixel.  meter: a frame's (S, K) per workgroup into the workspace.  adapt: ONE workgroup adds the
// partials of each frame of the group in order and carries the exposure through them; the exposure stays on the device.  map:
// exposure, curve, encode, one 4-byte store per pixel.  A fixed exposure needs only map.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "pt_stage.h"
#include "pt_stage_device.h"

namespace pttm {

constexpr int BLOCK = 256;                                   // lanes (pixels) per workgroup of every kernel
constexpr uint32_t METER_MIN = 0x35800000u;                  // bits(2^-20)
constexpr uint32_t METER_SPAN = 0x7F7FFFFFu - 0x35800000u;   // .. bits(FLT_MAX)
constexpr int K_SHIFT = 40;  // a lane's word is bits | 1 << 40: 256 lanes sum to S < 2^39 below the count

struct State {     // the session's device record
  float e;         // the exposure after the last frame
  uint32_t pad[3];
};

struct Image {
  const float* src;
  size_t src_stride;  // floats from frame to frame
  int pixel_stride;   // floats from pixel to pixel
  uint32_t pixels;
};

#pragma clang fp contract(off)

using pt_stage::lum;
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* red) { return pt_stage::block_sum<BLOCK>(v, red); }

// partials[frame][workgroup] = {S, K} of the workgroup's 256 pixels.  Every workgroup writes its word: nothing to clear.
__global__ void __launch_bounds__(BLOCK) meter_kernel(Image im, uint32_t blocks, ulonglong2* __restrict__ partials) {
  __shared__ uint64_t red[BLOCK / 64];
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, f = blockIdx.y;
  uint64_t word = 0;
  if (i < im.pixels) {
    const float* px = im.src + (size_t)f * im.src_stride + (size_t)i * (size_t)im.pixel_stride;
    const uint32_t b = __float_as_uint(lum(px[0], px[1], px[2]));
    if (b - METER_MIN <= METER_SPAN) word = (uint64_t)b | (1ull << K_SHIFT);  // finite and >= 2^-20
  }
  const uint64_t s = block_sum(word, red);
  if (threadIdx.x == 0) partials[(size_t)f * blocks + blockIdx.x] = make_ulonglong2(s & ((1ull << K_SHIFT) - 1), s >> K_SHIFT);
}

// One workgroup: for each frame of the group in order, (S, K) = the sum of its partials, then the definition's meter and adapt
// steps in thread 0.  exposures[frame] is what map_kernel reads; state->e carries over to the next call.
__global__ void __launch_bounds__(BLOCK) adapt_kernel(const ulonglong2* __restrict__ partials, uint32_t blocks, int frames, int first,
                                                      float key, float rate, State* __restrict__ state, float* __restrict__ exposures) {
  __shared__ uint64_t red[BLOCK / 64];
  float e = 1.0f;
  bool have = !first;
  if (threadIdx.x == 0 && have) e = state->e;
  for (int f = 0; f < frames; f++) {
    uint64_t S = 0, K = 0;
    const ulonglong2* p = partials + (size_t)f * blocks;
    for (uint32_t b = threadIdx.x; b < blocks; b += BLOCK) {
      const ulonglong2 v = p[b];
      S += v.x, K += v.y;  // (2^26 pixels x 2^31 < 2^64)
    }
    S = block_sum(S, red);
    K = block_sum(K, red);
    if (threadIdx.x == 0) {
      float target = have ? e : 1.0f;
      if (K != 0) target = key / __uint_as_float((uint32_t)(S / K));
      if (!have || rate == 1.0f) {
        e = target;
      } else {
        const float d = target - e;
        e = e + rate * d;
      }
      exposures[f] = e;
    }
    have = true;
  }
  if (threadIdx.x == 0) state->e = e;
}

template <int CURVE>
__device__ __forceinline__ void curve(float& r, float& g, float& b, float w2) {
  if (CURVE == PT_TONEMAP_REINHARD) {
    const float lx = lum(r, g, b);
    const float s = (1.0f + lx / w2) / (1.0f + lx);  // w2 = white * white
    r = r * s, g = g * s, b = b * s;
  } else if (CURVE == PT_TONEMAP_ACES) {
    r = (r * (2.51f * r + 0.03f)) / (r * (2.43f * r + 0.59f) + 0.14f);
    g = (g * (2.51f * g + 0.03f)) / (g * (2.43f * g + 0.59f) + 0.14f);
    b = (b * (2.51f * b + 0.03f)) / (b * (2.43f * b + 0.59f) + 0.14f);
  }
}

// the number of thresholds T[1 .. 255] <= y, in eight steps (T[0] is never read)
__device__ __forceinline__ uint32_t srgb_code(const float* T, float y) {
  uint32_t c = 0;
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1) c += T[c + s] <= y ? s : 0;
  return c;
}

template <int CURVE, int ENCODE>
__global__ void __launch_bounds__(BLOCK) map_kernel(Image im, const float* __restrict__ exposures, float fixed, float w2,
                                                    const float* __restrict__ table, uint32_t* __restrict__ dst, size_t dst_stride) {
  __shared__ float T[256];
  if (ENCODE == PT_ENCODE_SRGB) {
    T[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
  }
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, f = blockIdx.y;
  if (i >= im.pixels) return;
  const float e = exposures ? exposures[f] : fixed;
  const float* px = im.src + (size_t)f * im.src_stride + (size_t)i * (size_t)im.pixel_stride;
  float c[3] = {px[0], px[1], px[2]};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float x = c[k] * e;
    x = x > 0.0f ? x : 0.0f;  // (NaN becomes 0)
    c[k] = x < 65504.0f ? x : 65504.0f;
  }
  curve<CURVE>(c[0], c[1], c[2], w2);
  uint32_t packed = 255u << 24;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float y = c[k] < 1.0f ? c[k] : 1.0f;  // (NaN becomes 1)
    const uint32_t code = ENCODE == PT_ENCODE_SRGB ? srgb_code(T, y) : (uint32_t)(unsigned char)((double)y * 255.0);
    packed |= code << (8 * k);
  }
  dst[(size_t)f * dst_stride + i] = packed;
}

typedef void (*map_fn)(Image, const float*, float, float, const float*, uint32_t*, size_t);
static map_fn map_entry(int curve, int encode) {
  static const map_fn table[3][2] = {
      {map_kernel<PT_TONEMAP_CLAMP, PT_ENCODE_SRGB>, map_kernel<PT_TONEMAP_CLAMP, PT_ENCODE_LINEAR>},
      {map_kernel<PT_TONEMAP_REINHARD, PT_ENCODE_SRGB>, map_kernel<PT_TONEMAP_REINHARD, PT_ENCODE_LINEAR>},
      {map_kernel<PT_TONEMAP_ACES, PT_ENCODE_SRGB>, map_kernel<PT_TONEMAP_ACES, PT_ENCODE_LINEAR>},
  };
  return table[curve][encode];
}
}  // namespace pttm

using namespace pttm;

struct pt_tonemap {
  int width = 0, height = 0;
  pt_tonemap_opts opts{};
  uint32_t pixels = 0, blocks = 0;  // workgroups per frame
  int max_frames = 1;
  bool has_history = false;
  // fixed part: the sRGB table (256 floats, entry 0 unused) and the state; growing part: partials and exposures of a group
  float* d_table = nullptr;
  State* d_state = nullptr;
  ulonglong2* d_partials = nullptr;  // [max_frames][blocks]
  float* d_exposures = nullptr;      // [max_frames]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

using pt_stage::finite_f;

static void srgb_table(float out[255]) {
  for (int k = 1; k <= 255; k++) {
    const double u = ((double)k - 0.5) / 255.0;
    out[k - 1] = (float)(u <= 0.04045 ? u / 12.92 : pow((u + 0.055) / 1.055, 2.4));
  }
}

static size_t group_bytes(const pt_tonemap* t, int max_frames) {
  return (size_t)max_frames * t->blocks * sizeof(ulonglong2) + (size_t)max_frames * sizeof(float);
}
static size_t fixed_bytes() { return 256 * sizeof(float) + sizeof(State); }

static int check_frames(const char* who, int max_frames, int width, int height) {
  if (max_frames < 1) return pt_fail(PT_EINVAL, "%s: max_frames %d < 1", who, max_frames);
  if (max_frames > 65535) return pt_fail(PT_EINVAL, "%s: max_frames %d > 65535", who, max_frames);
  if ((int64_t)max_frames * width * height > ((int64_t)1 << 26))
    return pt_fail(PT_EINVAL, "%s: max_frames %d x %d x %d pixels exceeds 2^26", who, max_frames, width, height);
  return PT_OK;
}

// (every check before any launch: a refused call launches nothing and leaves the session as it was)
static int check_args(const char* who, const pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride,
                      const uint32_t* d_rgba8, size_t dst_stride_pixels) {
  if (!t) return pt_fail(PT_EINVAL, "%s: null tone mapper", who);
  if (!d_src) return pt_fail(PT_EINVAL, "%s: null d_src", who);
  if (!d_rgba8) return pt_fail(PT_EINVAL, "%s: null d_rgba8", who);
  if (n_frames < 1) return pt_fail(PT_EINVAL, "%s: n_frames %d < 1", who, n_frames);
  if (pixel_stride < 3 || pixel_stride > 64) return pt_fail(PT_EINVAL, "%s: pixel_stride %d outside 3 .. 64", who, pixel_stride);
  const size_t pixels = t->pixels;
  if (src_stride_floats < pixels * (size_t)pixel_stride)
    return pt_fail(PT_EINVAL, "%s: src_stride_floats %zu < width x height x pixel_stride = %zu", who, src_stride_floats,
                   pixels * (size_t)pixel_stride);
  if (dst_stride_pixels < pixels) return pt_fail(PT_EINVAL, "%s: dst_stride_pixels %zu < width x height = %zu", who, dst_stride_pixels, pixels);
  return PT_OK;
}

static int enqueue_frames(const char* who, pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride,
                          uint32_t* d_rgba8, size_t dst_stride_pixels, hipStream_t s) {
  const int rc = check_args(who, t, n_frames, d_src, src_stride_floats, pixel_stride, d_rgba8, dst_stride_pixels);
  if (rc != PT_OK) return rc;
  const bool automatic = t->opts.exposure == 0.0f;
  const map_fn map = map_entry(t->opts.curve, t->opts.encode);
  const float w2 = t->opts.white * t->opts.white;
  for (int f0 = 0; f0 < n_frames; f0 += t->max_frames) {
    const int n = n_frames - f0 < t->max_frames ? n_frames - f0 : t->max_frames;
    Image im{d_src + (size_t)f0 * src_stride_floats, src_stride_floats, pixel_stride, t->pixels};
    const dim3 grid(t->blocks, (unsigned)n), block(BLOCK);
    if (automatic) {
      hipLaunchKernelGGL(meter_kernel, grid, block, 0, s, im, t->blocks, t->d_partials);
      PT_HIP(hipGetLastError());
      hipLaunchKernelGGL(adapt_kernel, dim3(1), block, 0, s, (const ulonglong2*)t->d_partials, t->blocks, n, t->has_history ? 0 : 1,
                         t->opts.key, t->opts.adapt, t->d_state, t->d_exposures);
      PT_HIP(hipGetLastError());
      t->has_history = true;
    }
    hipLaunchKernelGGL(map, grid, block, 0, s, im, automatic ? (const float*)t->d_exposures : (const float*)nullptr, t->opts.exposure, w2,
                       (const float*)t->d_table, d_rgba8 + (size_t)f0 * dst_stride_pixels, dst_stride_pixels);
    PT_HIP(hipGetLastError());
  }
  return PT_OK;
}

static int run_timed(const char* who, pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride,
                     uint32_t* d_rgba8, size_t dst_stride_pixels, float* ms_out) {
  const int rc0 = check_args(who, t, n_frames, d_src, src_stride_floats, pixel_stride, d_rgba8, dst_stride_pixels);
  if (rc0 != PT_OK) return rc0;
  return pt_stage::run_timed(t->ev0, t->ev1, ms_out, [&] {
    return enqueue_frames(who, t, n_frames, d_src, src_stride_floats, pixel_stride, d_rgba8, dst_stride_pixels, nullptr);
  });
}

extern "C" {

void pt_tonemap_opts_default(pt_tonemap_opts* opts) {
  if (!opts) return;
  *opts = pt_tonemap_opts{};
  opts->curve = PT_TONEMAP_ACES, opts->encode = PT_ENCODE_SRGB;
  opts->exposure = 0.0f;
  opts->key = 0.18f, opts->white = 4.0f, opts->adapt = 1.0f;
  opts->max_frames = 1;
}

int pt_tonemap_srgb_table(float out[255]) {
  if (!out) return pt_fail(PT_EINVAL, "pt_tonemap_srgb_table: null output pointer");
  srgb_table(out);
  return PT_OK;
}

int pt_tonemap_destroy(pt_tonemap* t) {
  if (!t) return PT_OK;
  if (t->d_table) (void)hipFree(t->d_table);  // (the state lives behind the table)
  if (t->d_partials) (void)hipFree(t->d_partials);
  pt_stage::destroy_events(t);
  delete t;
  return PT_OK;
}

int pt_tonemap_create(int width, int height, const pt_tonemap_opts* opts, pt_tonemap** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_tonemap_create: null output pointer");
  *out = nullptr;
  pt_tonemap_opts o;
  if (opts) o = *opts;
  else pt_tonemap_opts_default(&o);
  int rc = pt_stage::check_frame_size("pt_tonemap_create", width, height);
  if (rc != PT_OK) return rc;
  if (o.curve < PT_TONEMAP_CLAMP || o.curve > PT_TONEMAP_ACES)
    return pt_fail(PT_EINVAL, "pt_tonemap_create: curve %d is none of PT_TONEMAP_CLAMP, _REINHARD, _ACES", o.curve);
  if (o.encode != PT_ENCODE_SRGB && o.encode != PT_ENCODE_LINEAR)
    return pt_fail(PT_EINVAL, "pt_tonemap_create: encode %d is neither PT_ENCODE_SRGB nor PT_ENCODE_LINEAR", o.encode);
  if (!(o.exposure >= 0.0f) || !finite_f(o.exposure))
    return pt_fail(PT_EINVAL, "pt_tonemap_create: exposure %g must be 0 (auto) or finite and > 0", (double)o.exposure);
  if (!(o.key > 0.0f) || !finite_f(o.key)) return pt_fail(PT_EINVAL, "pt_tonemap_create: key %g must be finite and > 0", (double)o.key);
  if (!(o.white >= 1e-18f && o.white <= 1e18f))
    return pt_fail(PT_EINVAL, "pt_tonemap_create: white %g outside 1e-18 .. 1e18 (its square must be a float)", (double)o.white);
  if (!(o.adapt > 0.0f && o.adapt <= 1.0f)) return pt_fail(PT_EINVAL, "pt_tonemap_create: adapt %g outside (0, 1]", (double)o.adapt);
  if ((rc = check_frames("pt_tonemap_create", o.max_frames, width, height)) != PT_OK) return rc;
  for (int k = 0; k < 2; k++)
    if (o.reserved[k] != 0) return pt_fail(PT_EINVAL, "pt_tonemap_create: reserved[%d] = %d must be 0", k, o.reserved[k]);
  if ((rc = pt_stage::check_device("pt_tonemap_create")) != PT_OK) return rc;
  pt_tonemap* t = new (std::nothrow) pt_tonemap();
  if (!t) return pt_fail(PT_ENOMEM, "pt_tonemap_create: out of host memory");
  t->width = width, t->height = height, t->opts = o;
  t->pixels = (uint32_t)width * (uint32_t)height;
  t->blocks = (t->pixels + BLOCK - 1) / BLOCK;
  t->max_frames = o.max_frames;
  float host[256 + sizeof(State) / sizeof(float)] = {};
  srgb_table(host + 1);
  host[256] = 1.0f;  // State::e
  hipError_t e = hipMalloc((void**)&t->d_table, fixed_bytes());
  if (e == hipSuccess) e = hipMemcpy(t->d_table, host, fixed_bytes(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_partials, group_bytes(t, t->max_frames));
  if ((rc = pt_stage::create_events("pt_tonemap_create", e, t, pt_tonemap_destroy)) != PT_OK) return rc;
  t->d_state = reinterpret_cast<State*>(t->d_table + 256);
  t->d_exposures = reinterpret_cast<float*>(t->d_partials + (size_t)t->max_frames * t->blocks);
  *out = t;
  return PT_OK;
}

int pt_tonemap_reset(pt_tonemap* t) {
  if (!t) return pt_fail(PT_EINVAL, "pt_tonemap_reset: null tone mapper");
  t->has_history = false;
  return PT_OK;
}

int pt_tonemap_workspace_bytes(const pt_tonemap* t, uint64_t* bytes) {
  if (!t || !bytes) return pt_fail(PT_EINVAL, "pt_tonemap_workspace_bytes: null %s", t ? "output pointer" : "tone mapper");
  *bytes = fixed_bytes() + group_bytes(t, t->max_frames);
  return PT_OK;
}

int pt_tonemap_reserve_frames(pt_tonemap* t, int max_frames) {
  if (!t) return pt_fail(PT_EINVAL, "pt_tonemap_reserve_frames: null tone mapper");
  int rc = check_frames("pt_tonemap_reserve_frames", max_frames, t->width, t->height);
  if (rc != PT_OK) return rc;
  if (max_frames <= t->max_frames) return PT_OK;
  const pt_stage::Buffer bufs[1] = {{(void**)&t->d_partials, group_bytes(t, max_frames), false}};  // (the state is not in this allocation)
  rc = pt_stage::grow_workspace("pt_tonemap_reserve_frames", bufs, "%d frames (%zu bytes)", max_frames, group_bytes(t, max_frames));
  if (rc != PT_OK) return rc;
  t->max_frames = max_frames;
  t->d_exposures = reinterpret_cast<float*>(t->d_partials + (size_t)max_frames * t->blocks);
  return PT_OK;
}

int pt_tonemap_enqueue(pt_tonemap* t, const float* d_src, int pixel_stride, uint32_t* d_rgba8, void* hip_stream) {
  if (!t) return pt_fail(PT_EINVAL, "pt_tonemap_enqueue: null tone mapper");
  return enqueue_frames("pt_tonemap_enqueue", t, 1, d_src, (size_t)t->pixels * 64, pixel_stride, d_rgba8, t->pixels, (hipStream_t)hip_stream);
}

int pt_tonemap_run(pt_tonemap* t, const float* d_src, int pixel_stride, uint32_t* d_rgba8, float* ms_out) {
  if (!t) return pt_fail(PT_EINVAL, "pt_tonemap_run: null tone mapper");
  return run_timed("pt_tonemap_run", t, 1, d_src, (size_t)t->pixels * 64, pixel_stride, d_rgba8, t->pixels, ms_out);
}

int pt_tonemap_enqueue_frames(pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride, uint32_t* d_rgba8,
                              size_t dst_stride_pixels, void* hip_stream) {
  return enqueue_frames("pt_tonemap_enqueue_frames", t, n_frames, d_src, src_stride_floats, pixel_stride, d_rgba8, dst_stride_pixels,
                        (hipStream_t)hip_stream);
}

int pt_tonemap_run_frames(pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride, uint32_t* d_rgba8,
                          size_t dst_stride_pixels, float* ms_out) {
  return run_timed("pt_tonemap_run_frames", t, n_frames, d_src, src_stride_floats, pixel_stride, d_rgba8, dst_stride_pixels, ms_out);
}

int pt_tonemap_exposure(pt_tonemap* t, float* out) {
  if (!t || !out) return pt_fail(PT_EINVAL, "pt_tonemap_exposure: null %s", t ? "output pointer" : "tone mapper");
  if (t->opts.exposure != 0.0f) {
    *out = t->opts.exposure;
    return PT_OK;
  }
  if (!t->has_history) {  // no frame since the session began or was reset
    *out = 1.0f;
    return PT_OK;
  }
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(out, &t->d_state->e, sizeof(float), hipMemcpyDeviceToHost));
  return PT_OK;
}

}  // extern "C"
