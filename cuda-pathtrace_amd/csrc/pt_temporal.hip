// pt_temporal.hip -- the temporal accumulator behind pt_temporal_* (include/ptcore.h): the temporal stage of SVGF in front of
// the feature-guided filter of pt_filter.hip.  Every pixel of a fly-through frame is carried back to the world through its mean
// depth, projected into the previous frame's camera, and blended with what the previous frames had accumulated there when depth,
// normal and albedo agree; the frame's variance channel becomes the variance of all the samples merged.  No counterpart in the
// reference.  DENOISER.md, "Temporal accumulation", states the definition; tests/temporal_model.py restates it in NumPy.
// EXACT code, unlike pt_filter.hip: no contraction, no rcp, IEEE divisions -- the kernel is held to the float32 model bit for bit.
//
// One kernel, one lane per pixel, one launch per frame (frame k reads what frame k-1 wrote).  The two cameras are kernel
// arguments; the history is three float4 images per pixel {colour, s2}, {normal, z}, {albedo, count}, two copies used
// ping-pong: a launch gathers four taps from one (16-byte loads) and writes the other.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "pt_stage.h"

namespace pttmp {

constexpr int BX = 32, BY = 8;  // workgroup: 32 columns x 8 rows, as pt_filter.hip

struct Params {
  int width, height;
  uint32_t pixels;
  int has_history;                         // 0: the frame passes through (first call, after a reset)
  float n;                                 // the frame's uniform sample count
  float fw, fh;                            // (float)width, (float)height
  float b0[3], e1[3], b2[3], e2[3];        // this frame: B0, B1 - B0, B2, B3 - B2 (float32 differences)
  float eye[3];
  float P[9], peye[3];                     // the previous frame: inverse of [B0 | B1-B0 | B2-B0], row-major, and its eye
  float cap, depth_tol, normal_tol, albedo_tol, min_weight;
};

#pragma clang fp contract(off)

__device__ __forceinline__ float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

__global__ void __launch_bounds__(BX* BY) accumulate_kernel(Params p, float* __restrict__ frame, const float4* __restrict__ hin,
                                                            float4* __restrict__ hout, uint32_t* __restrict__ counts) {
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const uint32_t W = (uint32_t)p.width, i = (uint32_t)y * W + (uint32_t)x;
  float* px = frame + (size_t)i * 14;
  const float cx = px[0], cy = px[1], cz = px[2];
  const float nx = px[3], ny = px[4], nz = px[5];
  const float ax = px[6], ay = px[7], az = px[8];
  const float z = px[9], s2c = px[10];

  float hx = 0.0f, hy = 0.0f, hz = 0.0f, hs2 = 0.0f, hN = 0.0f;
  if (p.has_history) {  // uniform
    // the renderer's primary direction of the unjittered pixel: the row is divided by the width, the column by the height
    const float sy = (float)x / p.fh, v = 1.0f - (float)y / p.fw;
    float X[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float a = p.b0[k] + sy * p.e1[k], b = p.b2[k] + sy * p.e2[k];
      const float d = a + v * (b - a);
      X[k] = p.eye[k] + d * z;
    }
    const float qx = X[0] - p.peye[0], qy = X[1] - p.peye[1], qz = X[2] - p.peye[2];
    const float al = (p.P[0] * qx + p.P[1] * qy) + p.P[2] * qz;
    const float be = (p.P[3] * qx + p.P[4] * qy) + p.P[5] * qz;
    const float ga = (p.P[6] * qx + p.P[7] * qy) + p.P[8] * qz;
    float cc = (be / al) * p.fh, rr = (1.0f - ga / al) * p.fw;
    // (every comparison fails for a NaN)
    const bool ok = z > 0.0f && al > 0.0f && cc > -1.0f && cc < p.fw && rr > -1.0f && rr < p.fh;
    cc = ok ? cc : 0.0f, rr = ok ? rr : 0.0f;  // so that the conversions below are defined
    const float r0f = floorf(rr), c0f = floorf(cc);
    const float fr = rr - r0f, fc = cc - c0f;
    const int r0 = (int)r0f, c0 = (int)c0f;  // -1 .. height - 1, -1 .. width - 1
    const float dtol = p.depth_tol * al;
    float ws = 0.0f, sx = 0.0f, sy2 = 0.0f, sz = 0.0f, ss = 0.0f, sn = 0.0f;
#pragma unroll
    for (int dr = 0; dr < 2; dr++) {
#pragma unroll
      for (int dc = 0; dc < 2; dc++) {
        const int tr = r0 + dr, tc = c0 + dc;
        const bool inside = tr >= 0 && tr < p.height && tc >= 0 && tc < p.width;
        // a tap outside the frame reads the clamped address and gets weight 0
        const uint32_t q = (uint32_t)min(max(tr, 0), p.height - 1) * W + (uint32_t)min(max(tc, 0), p.width - 1);
        const float4 t0 = hin[q], t1 = hin[p.pixels + q], t2 = hin[2 * p.pixels + q];
        const float wgt = (dr ? fr : 1.0f - fr) * (dc ? fc : 1.0f - fc);
        const float dax = t2.x - ax, day = t2.y - ay, daz = t2.z - az;
        const bool valid = ok & inside & (t2.w > 0.0f) & (fabsf(t1.w - al) <= dtol) &
                           ((t1.x * nx + t1.y * ny) + t1.z * nz >= p.normal_tol) &
                           ((dax * dax + day * day) + daz * daz <= p.albedo_tol);
        // an invalid tap contributes 0 to every sum: its values are selected away with its weight (0 * NaN is NaN, and a
        // history pixel that fails a stop may hold anything)
        const float w = valid ? wgt : 0.0f;
        const float tx = valid ? t0.x : 0.0f, ty = valid ? t0.y : 0.0f, tz = valid ? t0.z : 0.0f;
        const float ts = valid ? t0.w : 0.0f, tn = valid ? t2.w : 0.0f;
        ws = ws + w;
        sx = sx + w * tx, sy2 = sy2 + w * ty, sz = sz + w * tz;
        ss = ss + w * ts;
        sn = sn + w * tn;
      }
    }
    const bool keep = ws >= p.min_weight;
    hx = keep ? sx / ws : 0.0f, hy = keep ? sy2 / ws : 0.0f, hz = keep ? sz / ws : 0.0f;
    hs2 = keep ? ss / ws : 0.0f;
    hN = keep ? fminf(sn / ws, p.cap) : 0.0f;
  }

  const float tot = hN + p.n, k = p.n / tot;
  const float ox = hx + k * (cx - hx), oy = hy + k * (cy - hy), oz = hz + k * (cz - hz);
  const float delta = lum(cx, cy, cz) - lum(hx, hy, hz);
  const float merged = ((hs2 * fmaxf(hN - 1.0f, 0.0f) + s2c * (p.n - 1.0f)) + delta * delta * (hN * p.n / tot)) / (tot - 1.0f);
  const float os2 = hN > 0.0f && tot > 1.0f ? merged : s2c;

  px[0] = ox, px[1] = oy, px[2] = oz;
  px[10] = os2;
  hout[i] = make_float4(ox, oy, oz, os2);
  hout[p.pixels + i] = make_float4(nx, ny, nz, z);
  hout[2 * p.pixels + i] = make_float4(ax, ay, az, tot);
  if (counts) counts[i] = (uint32_t)floorf(tot + 0.5f);
}
}  // namespace pttmp

using namespace pttmp;

struct pt_temporal {
  int width = 0, height = 0;
  pt_temporal_opts opts{};
  float4* d_hist = nullptr;  // [2][3][pixels]
  int cur = 0;               // the copy that holds the history
  bool has_history = false;
  float P[9] = {}, eye[3] = {};  // the previous call's camera
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

using pt_stage::finite_f;

// The host step of the definition, in double, no contraction (CXXFLAGS): P = adj(M) / det for M = [B0 | B1-B0 | B2-B0].
static int camera_matrix(const char* who, const float basis[12], float P[9]) {
  double B[4][3], m[3][3];
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 3; k++) B[j][k] = (double)basis[3 * j + k];
  for (int k = 0; k < 3; k++) m[k][0] = B[0][k], m[k][1] = B[1][k] - B[0][k], m[k][2] = B[2][k] - B[0][k];
  double C[3][3];
  C[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
  C[0][1] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
  C[0][2] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  C[1][0] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
  C[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
  C[1][2] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
  C[2][0] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
  C[2][1] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
  C[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
  const double det = (m[0][0] * C[0][0] + m[0][1] * C[0][1]) + m[0][2] * C[0][2];
  if (!(det >= -1.7976931348623157e308 && det <= 1.7976931348623157e308) || det == 0.0)
    return pt_fail(PT_EINVAL, "%s: basis: the corner directions B0, B1 - B0, B2 - B0 have no finite non-zero determinant (%g)", who, det);
  const double tol = 1e-3 * sqrt((B[0][0] * B[0][0] + B[0][1] * B[0][1]) + B[0][2] * B[0][2]);
  for (int k = 0; k < 3; k++) {
    const double gap = fabs(((B[1][k] + B[2][k]) - B[0][k]) - B[3][k]);
    if (!(gap <= tol))
      return pt_fail(PT_EINVAL, "%s: basis: B1 + B2 - B0 - B3 is %g in component %d, beyond 1e-3 |B0| = %g: not the parallelogram of Camera", who,
                     gap, k, tol);
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) P[3 * i + j] = (float)(C[j][i] / det);
  return PT_OK;
}

static size_t ws_bytes(const pt_temporal* t) { return (size_t)2 * 3 * t->width * t->height * sizeof(float4); }

// (every check before any launch: a refused call launches nothing and leaves the session as it was)
static int check_args(const char* who, const pt_temporal* t, int n_frames, const float* d_frames, size_t frame_stride_floats,
                      const float* bases, const float* eyes, int samples) {
  if (!t) return pt_fail(PT_EINVAL, "%s: null accumulator", who);
  if (!d_frames) return pt_fail(PT_EINVAL, "%s: null d_frames", who);
  if (n_frames < 1) return pt_fail(PT_EINVAL, "%s: n_frames %d < 1", who, n_frames);
  const size_t pixels = (size_t)t->width * t->height;
  if (frame_stride_floats < pixels * 14)
    return pt_fail(PT_EINVAL, "%s: frame_stride_floats %zu < width x height x 14 = %zu", who, frame_stride_floats, pixels * 14);
  if (samples < 1) return pt_fail(PT_EINVAL, "%s: samples %d < 1", who, samples);
  if (!bases) return pt_fail(PT_EINVAL, "%s: null basis", who);
  if (!eyes) return pt_fail(PT_EINVAL, "%s: null eye", who);
  for (int f = 0; f < n_frames; f++) {
    for (int k = 0; k < 3; k++)
      if (!finite_f(eyes[3 * f + k])) return pt_fail(PT_EINVAL, "%s: eye[%d] of frame %d is not finite", who, k, f);
    float P[9];
    const int rc = camera_matrix(who, bases + 12 * f, P);
    if (rc != PT_OK) return rc;
  }
  return PT_OK;
}

static int enqueue_frames(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                          const float* eyes, int samples, uint32_t* d_counts, hipStream_t s) {
  int rc = check_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples);
  if (rc != PT_OK) return rc;
  Params p{};
  p.width = t->width, p.height = t->height;
  p.pixels = (uint32_t)t->width * (uint32_t)t->height;
  p.n = (float)samples;
  p.fw = (float)t->width, p.fh = (float)t->height;
  p.cap = t->opts.history_cap, p.depth_tol = t->opts.depth_tol, p.normal_tol = t->opts.normal_tol;
  p.albedo_tol = t->opts.albedo_tol, p.min_weight = t->opts.min_weight;
  const dim3 block(BX, BY), grid((unsigned)((p.width + BX - 1) / BX), (unsigned)((p.height + BY - 1) / BY));
  for (int f = 0; f < n_frames; f++) {
    const float* B = bases + 12 * f;
    for (int k = 0; k < 3; k++) {
      p.b0[k] = B[k], p.e1[k] = B[3 + k] - B[k], p.b2[k] = B[6 + k], p.e2[k] = B[9 + k] - B[6 + k];
      p.eye[k] = eyes[3 * f + k], p.peye[k] = t->eye[k];
    }
    for (int k = 0; k < 9; k++) p.P[k] = t->P[k];
    p.has_history = t->has_history ? 1 : 0;
    float4* hin = t->d_hist + (size_t)t->cur * 3 * p.pixels;
    float4* hout = t->d_hist + (size_t)(1 - t->cur) * 3 * p.pixels;
    // the count image is that of the last frame
    hipLaunchKernelGGL(accumulate_kernel, grid, block, 0, s, p, d_frames + (size_t)f * frame_stride_floats, (const float4*)hin, hout,
                       f == n_frames - 1 ? d_counts : (uint32_t*)nullptr);
    PT_HIP(hipGetLastError());
    (void)camera_matrix(who, B, t->P);  // (checked above)
    for (int k = 0; k < 3; k++) t->eye[k] = eyes[3 * f + k];
    t->cur = 1 - t->cur;
    t->has_history = true;
  }
  return PT_OK;
}

static int run_timed(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                     const float* eyes, int samples, uint32_t* d_counts, float* ms_out) {
  const int rc0 = check_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples);
  if (rc0 != PT_OK) return rc0;
  return pt_stage::run_timed(t->ev0, t->ev1, ms_out, [&] {
    return enqueue_frames(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, d_counts, nullptr);
  });
}

extern "C" {

void pt_temporal_opts_default(pt_temporal_opts* opts) {
  if (!opts) return;
  *opts = pt_temporal_opts{};
  opts->history_cap = 256.0f;
  opts->depth_tol = 0.02f, opts->normal_tol = 0.9f, opts->albedo_tol = 0.01f;
  opts->min_weight = 0.25f;
}

int pt_temporal_camera(const float basis[12], float P_out[9]) {
  if (!basis || !P_out) return pt_fail(PT_EINVAL, "pt_temporal_camera: null %s", basis ? "output pointer" : "basis");
  float P[9];
  const int rc = camera_matrix("pt_temporal_camera", basis, P);
  if (rc != PT_OK) return rc;
  for (int k = 0; k < 9; k++) P_out[k] = P[k];
  return PT_OK;
}

int pt_temporal_destroy(pt_temporal* t) {
  if (!t) return PT_OK;
  if (t->d_hist) (void)hipFree(t->d_hist);
  pt_stage::destroy_events(t);
  delete t;
  return PT_OK;
}

int pt_temporal_create(int width, int height, const pt_temporal_opts* opts, pt_temporal** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_temporal_create: null output pointer");
  *out = nullptr;
  pt_temporal_opts o;
  if (opts) o = *opts;
  else pt_temporal_opts_default(&o);
  int rc = pt_stage::check_frame_size("pt_temporal_create", width, height);
  if (rc != PT_OK) return rc;
  if (!(o.history_cap >= 1.0f)) return pt_fail(PT_EINVAL, "pt_temporal_create: history_cap %g must be >= 1", (double)o.history_cap);
  if (!(o.depth_tol > 0.0f) || !finite_f(o.depth_tol))
    return pt_fail(PT_EINVAL, "pt_temporal_create: depth_tol %g must be finite and > 0", (double)o.depth_tol);
  if (!(o.normal_tol >= -1.0f && o.normal_tol <= 1.0f))
    return pt_fail(PT_EINVAL, "pt_temporal_create: normal_tol %g outside -1 .. 1", (double)o.normal_tol);
  if (!(o.albedo_tol > 0.0f) || !finite_f(o.albedo_tol))
    return pt_fail(PT_EINVAL, "pt_temporal_create: albedo_tol %g must be finite and > 0", (double)o.albedo_tol);
  if (!(o.min_weight > 0.0f && o.min_weight <= 1.0f))
    return pt_fail(PT_EINVAL, "pt_temporal_create: min_weight %g outside (0, 1]", (double)o.min_weight);
  if (o.reserved != 0) return pt_fail(PT_EINVAL, "pt_temporal_create: reserved = %d must be 0", o.reserved);
  if ((rc = pt_stage::check_device("pt_temporal_create")) != PT_OK) return rc;
  pt_temporal* t = new (std::nothrow) pt_temporal();
  if (!t) return pt_fail(PT_ENOMEM, "pt_temporal_create: out of host memory");
  t->width = width, t->height = height, t->opts = o;
  const hipError_t e = hipMalloc((void**)&t->d_hist, ws_bytes(t));
  if ((rc = pt_stage::create_events("pt_temporal_create", e, t, pt_temporal_destroy)) != PT_OK) return rc;
  *out = t;
  return PT_OK;
}

int pt_temporal_reset(pt_temporal* t) {
  if (!t) return pt_fail(PT_EINVAL, "pt_temporal_reset: null accumulator");
  t->has_history = false;
  return PT_OK;
}

int pt_temporal_workspace_bytes(const pt_temporal* t, uint64_t* bytes) {
  if (!t || !bytes) return pt_fail(PT_EINVAL, "pt_temporal_workspace_bytes: null %s", t ? "output pointer" : "accumulator");
  *bytes = ws_bytes(t);
  return PT_OK;
}

int pt_temporal_enqueue(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                        void* hip_stream) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_enqueue: null %s", t ? "d_frame" : "accumulator");
  return enqueue_frames("pt_temporal_enqueue", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, d_counts,
                        (hipStream_t)hip_stream);
}

int pt_temporal_run(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                    float* ms_out) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_run: null %s", t ? "d_frame" : "accumulator");
  return run_timed("pt_temporal_run", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, d_counts, ms_out);
}

int pt_temporal_enqueue_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                               const float* eyes, int samples, uint32_t* d_counts, void* hip_stream) {
  return enqueue_frames("pt_temporal_enqueue_frames", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, d_counts,
                        (hipStream_t)hip_stream);
}

int pt_temporal_run_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                           const float* eyes, int samples, uint32_t* d_counts, float* ms_out) {
  return run_timed("pt_temporal_run_frames", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, d_counts, ms_out);
}

}  // extern "C"
