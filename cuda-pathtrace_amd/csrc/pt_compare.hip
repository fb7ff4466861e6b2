// pt_compare.hip -- the comparison session behind pt_compare_* (include/ptcore.h): how far an image is from its reference.  One
// pass over two device images gives the clamped MSE ("what a display shows"), the capped relMSE of the HDR values and the SSIM of
// the display luminances (11 x 11 Gaussian window, sigma 1.5, replicated edges), as three integer sums per frame that are exact
// in any order, plus two counts; an optional map keeps (m, r, s) per pixel.  No counterpart in the reference, which judges its
// 2-spp frames against its 20000-spp frames off the device.  DENOISER.md, "Frame comparison", states the definition;
// tests/compare_model.py restates it in NumPy.  EXACT code, like pt_temporal.hip and pt_tonemap.hip: no contraction, IEEE
// divisions, no transcendental on the device -- the kernels are held to the float32 model bit for bit.
//
// Two kernels.  tile: one workgroup per 16 x 16 output tile of a frame; it stages the 26 x 26 halo of (la, lb) in LDS (m and r
// of the tile's own pixels come from the registers on the way), filters the five quantities horizontally into a second LDS
// array, vertically out of it, and writes its four sums to the workspace.  sum: ONE workgroup adds the partials of each frame
// of the group into the frame's record.  No float atomics, no memset, no host synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "pt_stage.h"
#include "pt_stage_device.h"

namespace ptcmp {

constexpr int BLOCK = 256;         // lanes per workgroup of both kernels
constexpr int TILE = 16;           // output pixels per side of a tile
constexpr int TAPS = 11, R = 5;    // the window and its radius
constexpr int HALO = TILE + 2 * R; // 26
// Row pitch of the halo arrays in floats.  In the horizontal pass a 32-lane half of a wave is two tile rows of 16 lanes, each
// lane reading column c + tap of its row with a 4-byte read (32 banks): rows r and r + 1 must lie 16 banks apart, so the pitch
// is 16 modulo 32.  The staging writes one row per half (26 of 32 lanes), which is conflict-free at any pitch.
constexpr int PITCH = 48;
constexpr float X_MAX = 65504.0f, R_CAP = 1024.0f, R_EPS = 0.01f;
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // (rounded once, as the model's F(0.01) * F(0.01))

struct Images {
  const float *img, *ref;
  size_t img_stride, ref_stride;  // floats from frame to frame (ref_stride 0: one reference)
  int img_px, ref_px;             // floats from pixel to pixel
  int width, height;
  float* map;                     // may be null
  size_t map_stride;
};

struct Partial {  // of one workgroup
  uint64_t qm, qr, qs, counts;  // counts = saturated | nonfinite << 32
};

struct Record {  // of one frame; what pt_compare_result downloads
  uint64_t qm, qr;
  int64_t qs;
  uint64_t saturated, nonfinite;
};

struct Weights {
  float w[TAPS];
};

#pragma clang fp contract(off)

using pt_stage::lum;
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* red) { return pt_stage::block_sum<BLOCK>(v, red); }

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// partials[frame][tile] = the four sums of the tile's pixels.  Every workgroup writes its record: nothing to clear.
__global__ void __launch_bounds__(BLOCK) tile_kernel(Images im, Weights wt, uint32_t tiles_x, uint32_t tiles, Partial* __restrict__ partials) {
  __shared__ float s_la[HALO * PITCH], s_lb[HALO * PITCH];
  __shared__ float s_h[5][HALO * TILE];
  __shared__ uint64_t red[BLOCK / 64];
  const uint32_t f = blockIdx.y;
  const int x0 = (int)(blockIdx.x % tiles_x) * TILE, y0 = (int)(blockIdx.x / tiles_x) * TILE;
  const float* img = im.img + (size_t)f * im.img_stride;
  const float* ref = im.ref + (size_t)f * im.ref_stride;
  float* map = im.map ? im.map + (size_t)f * im.map_stride : nullptr;
  uint64_t qm = 0, qr = 0, counts = 0;

  // ---- stage: 26 rows of 32 lanes, 26 of them at work; coordinates clamp, so every read lies inside the frame
  for (int i = threadIdx.x; i < HALO * 32; i += BLOCK) {
    const int r = i >> 5, c = i & 31;
    if (c >= HALO) continue;
    const int gx = x0 - R + c, gy = y0 - R + r;
    const int cx = gx < 0 ? 0 : (gx < im.width ? gx : im.width - 1), cy = gy < 0 ? 0 : (gy < im.height ? gy : im.height - 1);
    const size_t p = (size_t)cy * (size_t)im.width + (size_t)cx;
    const float* pa = img + p * (size_t)im.img_px;
    const float* pb = ref + p * (size_t)im.ref_px;
    const float ca[3] = {pa[0], pa[1], pa[2]}, cb[3] = {pb[0], pb[1], pb[2]};
    float a[3], b[3], da[3], db[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float x = ca[k] > 0.0f ? ca[k] : 0.0f;  // (NaN becomes 0)
      a[k] = x < X_MAX ? x : X_MAX;
      x = cb[k] > 0.0f ? cb[k] : 0.0f;
      b[k] = x < X_MAX ? x : X_MAX;
      da[k] = a[k] < 1.0f ? a[k] : 1.0f;
      db[k] = b[k] < 1.0f ? b[k] : 1.0f;
    }
    s_la[r * PITCH + c] = lum(da[0], da[1], da[2]);
    s_lb[r * PITCH + c] = lum(db[0], db[1], db[2]);
    // the tile's own pixels: m and r
    if (r >= R && r < R + TILE && c >= R && c < R + TILE && gx < im.width && gy < im.height) {
      float tm[3], tr[3];
      uint32_t sat = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        float d = da[k] - db[k];
        tm[k] = d * d;
        d = a[k] - b[k];
        const float t = (d * d) / (b[k] * b[k] + R_EPS);
        sat += t < R_CAP ? 0u : 1u;
        tr[k] = t < R_CAP ? t : R_CAP;
      }
      const float m = (tm[0] + tm[1]) + tm[2], rr = (tr[0] + tr[1]) + tr[2];
      const bool fin = finite_bits(ca[0]) & finite_bits(ca[1]) & finite_bits(ca[2]) & finite_bits(cb[0]) & finite_bits(cb[1]) & finite_bits(cb[2]);
      qm += (uint64_t)floor((double)m * 17179869184.0);  // 2^34
      qr += (uint64_t)floor((double)rr * 16777216.0);    // 2^24
      counts += (uint64_t)sat + ((uint64_t)(fin ? 0u : 1u) << 32);
      if (map) {
        map[p * 3 + 0] = m;
        map[p * 3 + 1] = rr;
      }
    }
  }
  __syncthreads();

  // ---- horizontal: 26 rows x 16 columns, taps from the lowest offset to the highest, one add per tap
  for (int i = threadIdx.x; i < HALO * TILE; i += BLOCK) {
    const int r = i >> 4, c = i & 15;
    const float* ra = s_la + r * PITCH + c;
    const float* rb = s_lb + r * PITCH + c;
    float va = ra[0], vb = rb[0];
    float h0 = wt.w[0] * va, h1 = wt.w[0] * vb, h2 = wt.w[0] * (va * va), h3 = wt.w[0] * (vb * vb), h4 = wt.w[0] * (va * vb);
#pragma unroll
    for (int t = 1; t < TAPS; t++) {
      va = ra[t], vb = rb[t];
      h0 = h0 + wt.w[t] * va;
      h1 = h1 + wt.w[t] * vb;
      h2 = h2 + wt.w[t] * (va * va);
      h3 = h3 + wt.w[t] * (vb * vb);
      h4 = h4 + wt.w[t] * (va * vb);
    }
    s_h[0][i] = h0, s_h[1][i] = h1, s_h[2][i] = h2, s_h[3][i] = h3, s_h[4][i] = h4;
  }
  __syncthreads();

  // ---- vertical and SSIM: one lane per pixel of the tile
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  uint64_t qs = 0;
  if (x0 + tx < im.width && y0 + ty < im.height) {
    float e[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const float* col = s_h[q] + ty * TILE + tx;
      float v = wt.w[0] * col[0];
#pragma unroll
      for (int t = 1; t < TAPS; t++) v = v + wt.w[t] * col[t * TILE];
      e[q] = v;
    }
    const float mab = e[0] * e[1], maa = e[0] * e[0], mbb = e[1] * e[1];
    const float va = e[2] - maa, vb = e[3] - mbb, cab = e[4] - mab;
    const float num = (2.0f * mab + C1) * (2.0f * cab + C2);
    const float den = ((maa + mbb) + C1) * ((va + vb) + C2);
    const float s = num / den;
    qs = (uint64_t)(int64_t)floor((double)s * 4294967296.0);  // 2^32; the sum wraps as two's complement
    if (map) map[((size_t)(y0 + ty) * (size_t)im.width + (size_t)(x0 + tx)) * 3 + 2] = s;
  }

  qm = block_sum(qm, red);
  qr = block_sum(qr, red);
  qs = block_sum(qs, red);
  counts = block_sum(counts, red);
  if (threadIdx.x == 0) partials[(size_t)f * tiles + blockIdx.x] = Partial{qm, qr, qs, counts};
}

// One workgroup: records[frame] = the sum of the frame's partials, for each frame of the group.
__global__ void __launch_bounds__(BLOCK) sum_kernel(const Partial* __restrict__ partials, uint32_t tiles, int frames, Record* __restrict__ records) {
  __shared__ uint64_t red[BLOCK / 64];
  for (int f = 0; f < frames; f++) {
    uint64_t qm = 0, qr = 0, qs = 0, sat = 0, nonf = 0;
    const Partial* p = partials + (size_t)f * tiles;
    for (uint32_t b = threadIdx.x; b < tiles; b += BLOCK) {
      const Partial v = p[b];
      qm += v.qm, qr += v.qr, qs += v.qs;
      sat += v.counts & 0xFFFFFFFFull, nonf += v.counts >> 32;
    }
    qm = block_sum(qm, red);
    qr = block_sum(qr, red);
    qs = block_sum(qs, red);
    sat = block_sum(sat, red);
    nonf = block_sum(nonf, red);
    if (threadIdx.x == 0) records[f] = Record{qm, qr, (int64_t)qs, sat, nonf};
  }
}
}  // namespace ptcmp

using namespace ptcmp;

struct pt_compare {
  int width = 0, height = 0;
  uint32_t pixels = 0, tiles_x = 0, tiles = 0;  // workgroups per frame
  int max_frames = 1;
  int record_frames = 0;  // the records the workspace holds
  int last_frames = 0;    // frames of the last accepted call: what pt_compare_result may ask for
  Weights weights{};
  Partial* d_partials = nullptr;  // [max_frames][tiles]
  Record* d_records = nullptr;    // [record_frames]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// The eleven weights of the window: exp(-(k - 5)^2 / (2 sigma^2)) in double, divided by their sum (added from k = 0 up), then
// rounded to float32.
static void ssim_weights(float out[TAPS]) {
  double g[TAPS], sum = 0.0;
  for (int k = 0; k < TAPS; k++) {
    const double d = (double)(k - R);
    g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < TAPS; k++) out[k] = (float)(g[k] / sum);
}

static size_t partial_bytes(const pt_compare* c, int max_frames) { return (size_t)max_frames * c->tiles * sizeof(Partial); }
static size_t record_bytes(int frames) { return (size_t)frames * sizeof(Record); }

static int check_frames(const char* who, int max_frames, int width, int height) {
  if (max_frames < 1) return pt_fail(PT_EINVAL, "%s: max_frames %d < 1", who, max_frames);
  return pt_stage::check_batch(who, max_frames, width, height);
}

struct Call {
  int n_frames;
  const float* d_img;
  size_t img_stride_floats;
  int img_pixel_stride;
  const float* d_ref;
  size_t ref_stride_floats;
  int ref_pixel_stride;
  float* d_map;
  size_t map_stride_floats;
};

// (every check before any launch: a refused call launches nothing and leaves the session and its results as they were)
static int check_args(const char* who, const pt_compare* c, const Call& a) {
  if (!c) return pt_fail(PT_EINVAL, "%s: null comparison", who);
  if (!a.d_img) return pt_fail(PT_EINVAL, "%s: null d_img", who);
  if (!a.d_ref) return pt_fail(PT_EINVAL, "%s: null d_ref", who);
  if (a.n_frames < 1) return pt_fail(PT_EINVAL, "%s: n_frames %d < 1", who, a.n_frames);
  if (a.img_pixel_stride < 3 || a.img_pixel_stride > 64)
    return pt_fail(PT_EINVAL, "%s: img_pixel_stride %d outside 3 .. 64", who, a.img_pixel_stride);
  if (a.ref_pixel_stride < 3 || a.ref_pixel_stride > 64)
    return pt_fail(PT_EINVAL, "%s: ref_pixel_stride %d outside 3 .. 64", who, a.ref_pixel_stride);
  const size_t pixels = c->pixels;
  if (a.img_stride_floats < pixels * (size_t)a.img_pixel_stride)
    return pt_fail(PT_EINVAL, "%s: img_stride_floats %zu < width x height x img_pixel_stride = %zu", who, a.img_stride_floats,
                   pixels * (size_t)a.img_pixel_stride);
  if (a.ref_stride_floats != 0 && a.ref_stride_floats < pixels * (size_t)a.ref_pixel_stride)
    return pt_fail(PT_EINVAL, "%s: ref_stride_floats %zu is neither 0 (one reference) nor >= width x height x ref_pixel_stride = %zu", who,
                   a.ref_stride_floats, pixels * (size_t)a.ref_pixel_stride);
  if (a.d_map && a.map_stride_floats < pixels * 3)
    return pt_fail(PT_EINVAL, "%s: map_stride_floats %zu < width x height x 3 = %zu", who, a.map_stride_floats, pixels * 3);
  return PT_OK;
}

static int enqueue_frames(const char* who, pt_compare* c, const Call& a, hipStream_t s) {
  int rc = check_args(who, c, a);
  if (rc != PT_OK) return rc;
  if (a.n_frames > c->record_frames) {  // more frames than any call before: room for their records (waits for the device once)
    const pt_stage::Buffer bufs[1] = {{(void**)&c->d_records, record_bytes(a.n_frames), false}};
    rc = pt_stage::grow_workspace(who, bufs, "the records of %d frames (%zu bytes)", a.n_frames, record_bytes(a.n_frames));
    if (rc != PT_OK) return rc;
    c->record_frames = a.n_frames;
    c->last_frames = 0;  // (the old records went with the old buffer)
  }
  for (int f0 = 0; f0 < a.n_frames; f0 += c->max_frames) {
    const int n = a.n_frames - f0 < c->max_frames ? a.n_frames - f0 : c->max_frames;
    Images im{a.d_img + (size_t)f0 * a.img_stride_floats,
              a.d_ref + (size_t)f0 * a.ref_stride_floats,
              a.img_stride_floats,
              a.ref_stride_floats,
              a.img_pixel_stride,
              a.ref_pixel_stride,
              c->width,
              c->height,
              a.d_map ? a.d_map + (size_t)f0 * a.map_stride_floats : nullptr,
              a.map_stride_floats};
    hipLaunchKernelGGL(tile_kernel, dim3(c->tiles, (unsigned)n), dim3(BLOCK), 0, s, im, c->weights, c->tiles_x, c->tiles, c->d_partials);
    PT_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(BLOCK), 0, s, (const Partial*)c->d_partials, c->tiles, n, c->d_records + f0);
    PT_HIP(hipGetLastError());
  }
  c->last_frames = a.n_frames;
  return PT_OK;
}

static int run_timed(const char* who, pt_compare* c, const Call& a, float* ms_out) {
  const int rc0 = check_args(who, c, a);
  if (rc0 != PT_OK) return rc0;
  return pt_stage::run_timed(c->ev0, c->ev1, ms_out, [&] { return enqueue_frames(who, c, a, nullptr); });
}

static Call single(const pt_compare* c, const float* d_img, int img_pixel_stride, const float* d_ref, int ref_pixel_stride, float* d_map) {
  return Call{1, d_img, (size_t)c->pixels * 64, img_pixel_stride, d_ref, (size_t)c->pixels * 64, ref_pixel_stride, d_map, (size_t)c->pixels * 3};
}

extern "C" {

void pt_compare_opts_default(pt_compare_opts* opts) {
  if (!opts) return;
  *opts = pt_compare_opts{};
  opts->max_frames = 1;
}

int pt_compare_ssim_weights(float out[11]) {
  if (!out) return pt_fail(PT_EINVAL, "pt_compare_ssim_weights: null output pointer");
  ssim_weights(out);
  return PT_OK;
}

int pt_compare_destroy(pt_compare* c) {
  if (!c) return PT_OK;
  if (c->d_partials) (void)hipFree(c->d_partials);
  if (c->d_records) (void)hipFree(c->d_records);
  pt_stage::destroy_events(c);
  delete c;
  return PT_OK;
}

int pt_compare_create(int width, int height, const pt_compare_opts* opts, pt_compare** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_compare_create: null output pointer");
  *out = nullptr;
  pt_compare_opts o;
  if (opts) o = *opts;
  else pt_compare_opts_default(&o);
  int rc = pt_stage::check_frame_size("pt_compare_create", width, height);
  if (rc != PT_OK) return rc;
  if ((rc = check_frames("pt_compare_create", o.max_frames, width, height)) != PT_OK) return rc;
  for (int k = 0; k < 3; k++)
    if (o.reserved[k] != 0) return pt_fail(PT_EINVAL, "pt_compare_create: reserved[%d] = %d must be 0", k, o.reserved[k]);
  if ((rc = pt_stage::check_device("pt_compare_create")) != PT_OK) return rc;
  pt_compare* c = new (std::nothrow) pt_compare();
  if (!c) return pt_fail(PT_ENOMEM, "pt_compare_create: out of host memory");
  c->width = width, c->height = height;
  c->pixels = (uint32_t)width * (uint32_t)height;
  c->tiles_x = (uint32_t)(width + TILE - 1) / TILE;
  c->tiles = c->tiles_x * ((uint32_t)(height + TILE - 1) / TILE);
  c->max_frames = c->record_frames = o.max_frames;
  ssim_weights(c->weights.w);
  hipError_t e = hipMalloc((void**)&c->d_partials, partial_bytes(c, c->max_frames));
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_records, record_bytes(c->record_frames));
  if ((rc = pt_stage::create_events("pt_compare_create", e, c, pt_compare_destroy)) != PT_OK) return rc;
  *out = c;
  return PT_OK;
}

int pt_compare_workspace_bytes(const pt_compare* c, uint64_t* bytes) {
  if (!c || !bytes) return pt_fail(PT_EINVAL, "pt_compare_workspace_bytes: null %s", c ? "output pointer" : "comparison");
  *bytes = partial_bytes(c, c->max_frames) + record_bytes(c->record_frames);
  return PT_OK;
}

int pt_compare_reserve_frames(pt_compare* c, int max_frames) {
  if (!c) return pt_fail(PT_EINVAL, "pt_compare_reserve_frames: null comparison");
  int rc = check_frames("pt_compare_reserve_frames", max_frames, c->width, c->height);
  if (rc != PT_OK) return rc;
  if (max_frames <= c->max_frames) return PT_OK;
  const pt_stage::Buffer bufs[1] = {{(void**)&c->d_partials, partial_bytes(c, max_frames), false}};  // (the records stay)
  rc = pt_stage::grow_workspace("pt_compare_reserve_frames", bufs, "%d frames (%zu bytes)", max_frames, partial_bytes(c, max_frames));
  if (rc != PT_OK) return rc;
  c->max_frames = max_frames;
  return PT_OK;
}

int pt_compare_enqueue(pt_compare* c, const float* d_img, int img_pixel_stride, const float* d_ref, int ref_pixel_stride, float* d_map,
                       void* hip_stream) {
  if (!c) return pt_fail(PT_EINVAL, "pt_compare_enqueue: null comparison");
  return enqueue_frames("pt_compare_enqueue", c, single(c, d_img, img_pixel_stride, d_ref, ref_pixel_stride, d_map), (hipStream_t)hip_stream);
}

int pt_compare_run(pt_compare* c, const float* d_img, int img_pixel_stride, const float* d_ref, int ref_pixel_stride, float* d_map,
                   float* ms_out) {
  if (!c) return pt_fail(PT_EINVAL, "pt_compare_run: null comparison");
  return run_timed("pt_compare_run", c, single(c, d_img, img_pixel_stride, d_ref, ref_pixel_stride, d_map), ms_out);
}

int pt_compare_enqueue_frames(pt_compare* c, int n_frames, const float* d_img, size_t img_stride_floats, int img_pixel_stride,
                              const float* d_ref, size_t ref_stride_floats, int ref_pixel_stride, float* d_map, size_t map_stride_floats,
                              void* hip_stream) {
  return enqueue_frames("pt_compare_enqueue_frames", c,
                        Call{n_frames, d_img, img_stride_floats, img_pixel_stride, d_ref, ref_stride_floats, ref_pixel_stride, d_map, map_stride_floats},
                        (hipStream_t)hip_stream);
}

int pt_compare_run_frames(pt_compare* c, int n_frames, const float* d_img, size_t img_stride_floats, int img_pixel_stride, const float* d_ref,
                          size_t ref_stride_floats, int ref_pixel_stride, float* d_map, size_t map_stride_floats, float* ms_out) {
  return run_timed("pt_compare_run_frames", c,
                   Call{n_frames, d_img, img_stride_floats, img_pixel_stride, d_ref, ref_stride_floats, ref_pixel_stride, d_map, map_stride_floats},
                   ms_out);
}

int pt_compare_result(pt_compare* c, int frame_index, pt_compare_values* out) {
  if (!c || !out) return pt_fail(PT_EINVAL, "pt_compare_result: null %s", c ? "output pointer" : "comparison");
  if (frame_index < 0 || frame_index >= c->last_frames)
    return pt_fail(PT_EINVAL, "pt_compare_result: frame_index %d outside the last call's %d frames", frame_index, c->last_frames);
  Record r;
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(&r, c->d_records + frame_index, sizeof(Record), hipMemcpyDeviceToHost));
  const double px = (double)c->pixels;
  out->sum_mse = r.qm, out->sum_relmse = r.qr, out->sum_ssim = r.qs;
  out->pixels = c->pixels, out->saturated = r.saturated, out->nonfinite = r.nonfinite;
  out->mse = (double)r.qm / 17179869184.0 / (3.0 * px);
  out->rms = sqrt(out->mse);
  out->psnr = out->mse > 0.0 ? -10.0 * log10(out->mse) : (double)INFINITY;
  out->relmse = (double)r.qr / 16777216.0 / (3.0 * px);
  out->ssim = (double)r.qs / 4294967296.0 / px;
  return PT_OK;
}

}  // extern "C"
