// pt_temporal.hip -- the temporal accumulator behind pt_temporal_* (include/ptcore.h): the temporal stage of SVGF in front of
// the feature-guided filter of pt_filter.hip.  Every pixel of a fly-through frame is carried back to the world through its mean
// depth, projected into the previous frame's camera, and blended with what the previous frames had accumulated there when depth,
// normal and albedo agree; the frame's variance channel becomes the variance of all the samples merged.  No counterpart in the
// reference.  DENOISER.md, "Temporal accumulation", states the definition; tests/temporal_model.py restates it in NumPy.
// EXACT code, unlike pt_filter.hip: no contraction, no rcp, IEEE divisions -- the kernel is held to the float32 model bit for bit.
//
// One accumulate kernel, one lane per pixel, one launch per frame (frame k reads what frame k-1 wrote).  The two cameras are
// kernel arguments; the history is three float4 images per pixel {colour, s2}, {normal, z}, {albedo, count}, two copies used
// ping-pong: a launch gathers four taps from one (16-byte loads) and writes the other.
// Moving spheres (DENOISER.md, "Moving spheres"; tests/temporal_motion_model.py): the MOTION instantiation of that kernel takes a
// per-pixel motion image and carries the world point back by it before the previous camera looks; motion_kernel builds such an
// image from the spheres of this frame and of the previous one, which the _scene calls remember on the host.
// Responsive history (DENOISER.md, "Responsive history"; tests/temporal_antilag_model.py): the FAST instantiations of the
// accumulate kernel carry a second, short history {colour, count} through the same four taps, and rectify_kernel clamps the long
// history's colour into the range that short history shows in the (2R+1)^2 window around the pixel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

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

// Component k of the renderer's primary direction of the unjittered pixel (row y, column x): the row is divided by the width,
// the column by the height: sy = column / fh, v = 1 - row / fw, and the two lerps over (b0, e1 = B1 - B0, b2, e2 = B3 - B2).
// (Scalars by value: handed the parameter struct by reference, the compiler schedules the accumulate kernel differently.)
__device__ __forceinline__ float primary_direction(float b0, float e1, float b2, float e2, float sy, float v) {
  const float a = b0 + sy * e1, b = b2 + sy * e2;
  return a + v * (b - a);
}

template <class T, class... REST>
__device__ __forceinline__ T first(T a, REST...) {
  return a;
}

template <int N, class T, class... REST>
__device__ __forceinline__ auto pick(T a, REST... rest) {
  if constexpr (N == 0) return a;
  else return pick<N - 1>(rest...);
}

// MOTION: one more argument, `motion`, holds {mx, my, mz, w} per pixel (motion_kernel below) and the world point is carried back
// by m before the previous camera looks at it.  accumulate_kernel<false> takes no such argument: it has the signature, and
// instruction for instruction the code, that the kernel had before it became a template.
// FAST: three more arguments behind that, `fin`, `fout` (the fast history read and written, one float4 {colour, count} per pixel)
// and `fast_cap` -- in the pack and not in Params, so that the kernels without them keep their argument layout and their code.
template <bool MOTION, class... IMAGE>
__global__ void __launch_bounds__(BX* BY) accumulate_kernel(Params p, float* __restrict__ frame, const float4* __restrict__ hin,
                                                            float4* __restrict__ hout, uint32_t* __restrict__ counts, IMAGE... motion) {
  constexpr int NM = MOTION ? 1 : 0;
  constexpr bool FAST = sizeof...(IMAGE) == NM + 3;
  static_assert(sizeof...(IMAGE) == NM || FAST, "accumulate_kernel<MOTION[, const float4* motion][, const float4* fin, float4* fout, float fast_cap]>");
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const uint32_t W = (uint32_t)p.width, i = (uint32_t)y * W + (uint32_t)x;
  float* px = frame + (size_t)i * 14;
  const float cx = px[0], cy = px[1], cz = px[2];
  const float nx = px[3], ny = px[4], nz = px[5];
  const float ax = px[6], ay = px[7], az = px[8];
  const float z = px[9], s2c = px[10];

  float hx = 0.0f, hy = 0.0f, hz = 0.0f, hs2 = 0.0f, hN = 0.0f;
  float fx = 0.0f, fy = 0.0f, fz = 0.0f, fN = 0.0f;  // FAST: the fast history of the pixel
  if (p.has_history) {  // uniform
    const float sy = (float)x / p.fh, v = 1.0f - (float)y / p.fw;
    float X[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float d = primary_direction(p.b0[k], p.e1[k], p.b2[k], p.e2[k], sy, v);
      X[k] = p.eye[k] + d * z;
    }
    if constexpr (MOTION) {  // where the surface point was one frame ago
      const float4 m = first(motion...)[i];
      X[0] = X[0] - m.x, X[1] = X[1] - m.y, X[2] = X[2] - m.z;
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
    float gx = 0.0f, gy = 0.0f, gz = 0.0f, gn = 0.0f;
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
        if constexpr (FAST) {  // the same taps, the same weights: all four components selected, never multiplied
          const float4 tf = pick<NM>(motion...)[q];
          const float ux = valid ? tf.x : 0.0f, uy = valid ? tf.y : 0.0f, uz = valid ? tf.z : 0.0f, un = valid ? tf.w : 0.0f;
          gx = gx + w * ux, gy = gy + w * uy, gz = gz + w * uz;
          gn = gn + w * un;
        }
      }
    }
    const bool keep = ws >= p.min_weight;
    hx = keep ? sx / ws : 0.0f, hy = keep ? sy2 / ws : 0.0f, hz = keep ? sz / ws : 0.0f;
    hs2 = keep ? ss / ws : 0.0f;
    hN = keep ? fminf(sn / ws, p.cap) : 0.0f;
    if constexpr (FAST) {
      fx = keep ? gx / ws : 0.0f, fy = keep ? gy / ws : 0.0f, fz = keep ? gz / ws : 0.0f;
      fN = keep ? fminf(gn / ws, pick<NM + 2>(motion...)) : 0.0f;
    }
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
  if constexpr (FAST) {
    const float ftot = fN + p.n, kf = p.n / ftot;
    pick<NM + 1>(motion...)[i] = make_float4(fx + kf * (cx - fx), fy + kf * (cy - fy), fz + kf * (cz - fz), ftot);
  }
}

// ---- rectify: clamp the long history's colour into the fast history's neighbourhood range --------------------------------------
// One lane per pixel.  The workgroup stages the (BX + 2R) x (BY + 2R) tile of the fast image that its windows cover in LDS
// (38 x 14 float4 = 8.3 KB at R = 3); a tap outside the frame is FLAGGED there (.w = -1: a fast count is >= n >= 1), not clamped
// to the edge, and does not count.  The staging loop and the barrier are uniform over the workgroup: lanes outside the frame stage
// with the others and leave after the barrier.  Each lane then walks its window in row-major order, unrolled by R, so the sums
// are the definition's: sequential from +0, every product rounded before it is added.
struct RectifyParams {
  int width, height;
  uint32_t pixels;
  float k;  // clamp_sigma
};

__device__ __forceinline__ float rectify_channel(float x, float s1, float s2, float m, float k) {
  const float mu = s1 / m;
  const float v = s2 / m - mu * mu;
  const float var = v > 0.0f ? v : 0.0f;  // (a NaN gives 0)
  const float sd = k * sqrtf(var);  // (IEEE: the compiler expands it with its fix-up, as in pt_device.h)
  const float lo = mu - sd, hi = mu + sd;
  return x < lo ? lo : (x > hi ? hi : x);  // (NaN bounds pass x)
}

template <int R>
__global__ void __launch_bounds__(BX* BY) rectify_kernel(RectifyParams p, float* __restrict__ frame, const float4* __restrict__ fast,
                                                         float4* __restrict__ hist) {
  constexpr int TW = BX + 2 * R, TH = BY + 2 * R;
  __shared__ float4 tile[TH * TW];
  const int x0 = blockIdx.x * BX - R, y0 = blockIdx.y * BY - R;
  const int lane = threadIdx.y * BX + threadIdx.x;
  for (int j = lane; j < TH * TW; j += BX * BY) {  // (uniform bounds)
    const int ty = j / TW, tx = j - ty * TW;
    const int gx = x0 + tx, gy = y0 + ty;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (gx >= 0 && gx < p.width && gy >= 0 && gy < p.height) t = fast[(uint32_t)gy * (uint32_t)p.width + (uint32_t)gx];
    tile[j] = t;
  }
  __syncthreads();
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
  const float ftot = tile[(threadIdx.y + R) * TW + threadIdx.x + R].w;
  const float tot = hist[2 * p.pixels + i].w;
  if (!(tot > ftot)) return;  // inactive: the long history is no longer than the fast one, nothing is written
  float m = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
  for (int dy = 0; dy <= 2 * R; dy++) {
#pragma unroll
    for (int dx = 0; dx <= 2 * R; dx++) {
      const float4 t = tile[(threadIdx.y + dy) * TW + threadIdx.x + dx];
      const bool in = !(t.w < 0.0f);
      m = in ? m + 1.0f : m;
      ax = in ? ax + t.x : ax, ay = in ? ay + t.y : ay, az = in ? az + t.z : az;
      bx = in ? bx + t.x * t.x : bx, by = in ? by + t.y * t.y : by, bz = in ? bz + t.z * t.z : bz;
    }
  }
  const float4 c = hist[i];
  const float ox = rectify_channel(c.x, ax, bx, m, p.k), oy = rectify_channel(c.y, ay, by, m, p.k), oz = rectify_channel(c.z, az, bz, m, p.k);
  float* px = frame + (size_t)i * 14;
  px[0] = ox, px[1] = oy, px[2] = oz;
  hist[i] = make_float4(ox, oy, oz, c.w);
}

// ---- the motion image ---------------------------------------------------------------------------------------------------
// Which sphere does the centre ray of a pixel hit, and how far has that sphere moved since the previous frame?  One lane per
// pixel; the spheres of this frame {x, y, z, radius} go through LDS MOTION_CHUNK at a time (the staging and the loop bounds are
// uniform over the workgroup, the LDS reads are broadcasts), brute force: one primary ray per pixel needs no grid.  The search
// is the reference's intersectSphere / intersectScene (src/pathtrace.cu:72-107) literally -- the direction not normalised,
// double where its literals force double, the first of equal roots wins -- as tests/numpy_restatement.py states it.
constexpr int MOTION_CHUNK = PT_MOTION_CHUNK;
static_assert(MOTION_CHUNK == BX * BY, "one sphere per lane and round of the staging");

struct MotionParams {
  int width, height, n;
  float fw, fh;
  float b0[3], e1[3], b2[3], e2[3];
  float eye[3];
};

__global__ void __launch_bounds__(BX* BY) motion_kernel(MotionParams p, const float4* __restrict__ now, const float4* __restrict__ prev,
                                                        float4* __restrict__ out) {
  __shared__ float4 staged[MOTION_CHUNK];
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  const int lane = threadIdx.y * BX + threadIdx.x;
  const bool live = x < p.width && y < p.height;  // (a lane outside the frame stages and waits with the others)
  const float sy = (float)x / p.fh, v = 1.0f - (float)y / p.fw;
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = primary_direction(p.b0[k], p.e1[k], p.b2[k], p.e2[k], sy, v);
  const float a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];  // :74
  float tNearest = 1000000.0f;
  int idx = -1;
  for (int base = 0; base < p.n; base += MOTION_CHUNK) {
    const int m = min(MOTION_CHUNK, p.n - base);
    if (lane < m) staged[lane] = now[base + lane];
    __syncthreads();
    for (int j = 0; j < m; j++) {
      const float4 s = staged[j];
      const float ox = p.eye[0] - s.x, oy = p.eye[1] - s.y, oz = p.eye[2] - s.z;  // :73
      const float b = (float)(2.0 * (double)((d[0] * ox + d[1] * oy) + d[2] * oz));  // :75
      const float c = ((ox * ox + oy * oy) + oz * oz) - s.w * s.w;                  // :76
      const float bb = b * b;
      const float det = bb - (4.0f * a) * c;  // :77
      if (det >= 0.0f) {                      // :79
        const double root = sqrt((double)bb - (4.0 * (double)a) * (double)c), den = 2.0 * (double)a;
        const float tNear = (float)(((double)(-b) - root) / den), tFar = (float)(((double)(-b) + root) / den);  // :80-81
        const float t = tNear > 0.0f && tFar > 0.0f ? fminf(tNear, tFar) : tNear > 0.0f ? tNear : tFar;      // :82-87
        if (t > 0.0f && t < tNearest) tNearest = t, idx = base + j;  // :99
      }
    }
    __syncthreads();
  }
  if (!live) return;
  float4 r = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if (idx >= 0) {
    const float4 pn = now[idx], pp = prev[idx];
    r = make_float4(pn.x - pp.x, pn.y - pp.y, pn.z - pp.z, (float)idx);
  }
  out[(size_t)y * p.width + x] = r;
}
}  // namespace pttmp

using namespace pttmp;

constexpr int RING = 4;      // pinned staging slots of the spheres
constexpr int RETIRED = 20;  // staging buffers a session can outgrow (the capacity doubles: 17 at the most)

struct pt_temporal {
  int width = 0, height = 0;
  pt_temporal_opts opts{};
  float4* d_hist = nullptr;  // [2][3][pixels]
  int cur = 0;               // the copy that holds the history
  bool has_history = false;
  float P[9] = {}, eye[3] = {};  // the previous call's camera
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // what the motion calls need, allocated by the first of them that does
  float4* d_motion = nullptr;   // [pixels], the _scene calls' motion image
  float4* d_spheres = nullptr;  // [2][sphere_cap]: {pos, radius} of this frame, {pos, -} of the previous one
  float4* h_spheres = nullptr;  // pinned, [RING][2][sphere_cap]
  int sphere_cap = 0;
  float4 *retired_d[RETIRED] = {}, *retired_h[RETIRED] = {};  // outgrown staging buffers, freed with the session
  int n_retired = 0;
  hipEvent_t slot_done[RING] = {};  // the copy out of a slot has run
  bool slot_used[RING] = {};
  int next_slot = 0;
  pt_sphere* scene = nullptr;  // host copy of the previous _scene call's spheres, [scene_cap]
  int scene_n = 0, scene_cap = 0;
  bool has_scene = false;
  // responsive history (pt_temporal_set_antilag): off while antilag.fast_cap == 0
  pt_temporal_antilag_opts antilag{};
  float4* d_fast = nullptr;  // [2][pixels] {fast colour, fast count}, allocated by the first call that switches on
  int fcur = 0;              // the copy the last call wrote
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

static size_t hist_bytes(const pt_temporal* t) { return (size_t)2 * 3 * t->width * t->height * sizeof(float4); }
static size_t motion_bytes(const pt_temporal* t) { return (size_t)t->width * t->height * sizeof(float4); }
static size_t fast_bytes(const pt_temporal* t) { return (size_t)2 * t->width * t->height * sizeof(float4); }
static size_t ws_bytes(const pt_temporal* t) {
  return hist_bytes(t) + (t->d_motion ? motion_bytes(t) : 0) + (t->d_fast ? fast_bytes(t) : 0);
}

// Everything pt_temporal_set_antilag checks about its options; no device.
static int check_antilag(const char* who, const pt_temporal_antilag_opts* o, float history_cap) {
  if (!o) return pt_fail(PT_EINVAL, "%s: null opts", who);
  if (o->fast_cap != 0.0f && !(o->fast_cap >= 1.0f && o->fast_cap < history_cap))
    return pt_fail(PT_EINVAL, "%s: fast_cap %g must be 0 (off) or >= 1 and < history_cap = %g", who, (double)o->fast_cap, (double)history_cap);
  if (!(o->clamp_sigma > 0.0f) || !finite_f(o->clamp_sigma))
    return pt_fail(PT_EINVAL, "%s: clamp_sigma %g must be finite and > 0", who, (double)o->clamp_sigma);
  if (o->clamp_radius < 1 || o->clamp_radius > 3) return pt_fail(PT_EINVAL, "%s: clamp_radius %d outside 1 .. 3", who, o->clamp_radius);
  if (o->reserved != 0) return pt_fail(PT_EINVAL, "%s: reserved = %d must be 0", who, o->reserved);
  return PT_OK;
}

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

// ---- the spheres of the motion calls: host checks, staging, the launch ------------------------------------------------------

static int check_sphere_count(const char* who, int n) {
  if (n < 1 || n > 65535) return pt_fail(PT_EINVAL, "%s: n %d outside 1 .. 65535", who, n);
  return PT_OK;
}

static int check_sphere_fields(const char* who, const char* what, const pt_sphere* s, int n) {
  for (int i = 0; i < n; i++) {
    const float* f = &s[i].radius;  // radius, pos[3], emission[3], color[3]: ten floats
    static const char* const names[10] = {"radius", "pos[0]", "pos[1]", "pos[2]", "emission[0]", "emission[1]", "emission[2]",
                                          "color[0]", "color[1]", "color[2]"};
    for (int k = 0; k < 10; k++)
      if (!finite_f(f[k])) return pt_fail(PT_EINVAL, "%s: %s: %s of sphere %d is not finite", who, what, names[k], i);
  }
  return PT_OK;
}
static_assert(sizeof(pt_sphere) == 10 * sizeof(float), "pt_sphere is ten floats");

static int check_sphere_radii(const char* who, const char* what, const pt_sphere* now, const pt_sphere* prev, int n) {
  for (int i = 0; i < n; i++)
    if (memcmp(&now[i].radius, &prev[i].radius, sizeof(float)) != 0)
      return pt_fail(PT_EINVAL, "%s: %s: the radius of sphere %d changes from %g to %g, which is no rigid translation: reset the session", who,
                     what, i, (double)prev[i].radius, (double)now[i].radius);
  return PT_OK;
}

static int check_camera(const char* who, const float* basis, const float* eye) {
  if (!basis) return pt_fail(PT_EINVAL, "%s: null basis", who);
  if (!eye) return pt_fail(PT_EINVAL, "%s: null eye", who);
  for (int k = 0; k < 3; k++)
    if (!finite_f(eye[k])) return pt_fail(PT_EINVAL, "%s: eye[%d] is not finite", who, k);
  float P[9];
  return camera_matrix(who, basis, P);
}

// Everything pt_temporal_motion checks about its host arguments; no device.
static int check_motion_args(const char* who, const pt_sphere* h_now, const pt_sphere* h_prev, int n, const float* basis, const float* eye) {
  if (!h_now) return pt_fail(PT_EINVAL, "%s: null h_now", who);
  if (!h_prev) return pt_fail(PT_EINVAL, "%s: null h_prev", who);
  int rc = check_sphere_count(who, n);
  if (rc == PT_OK) rc = check_sphere_fields(who, "h_now", h_now, n);
  if (rc == PT_OK) rc = check_sphere_fields(who, "h_prev", h_prev, n);
  if (rc == PT_OK) rc = check_sphere_radii(who, "h_now", h_now, h_prev, n);
  if (rc == PT_OK) rc = check_camera(who, basis, eye);
  return rc;
}

// Room for n spheres in the staging buffers.  Nothing waits for the device: work already enqueued may still read the old
// buffers, so they are retired, not freed -- pt_temporal_destroy frees them.  The capacity at least doubles (up to the 65535
// spheres a call may have), so a session retires at most RETIRED pairs.  A failure frees what it got and leaves the session as
// it was.
static int ensure_staging(const char* who, pt_temporal* t, int n) {
  if (n <= t->sphere_cap) return PT_OK;
  const int cap = max(n, min(2 * t->sphere_cap, 65535));
  float4 *d = nullptr, *h = nullptr;
  const size_t bytes = (size_t)2 * cap * sizeof(float4);
  hipError_t e = t->n_retired < RETIRED ? hipSuccess : hipErrorOutOfMemory;  // (unreachable: 1 -> 65535 is 16 doublings)
  if (e == hipSuccess) e = hipMalloc((void**)&d, bytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h, RING * bytes, hipHostMallocDefault);
  for (int k = 0; k < RING; k++)
    if (e == hipSuccess && !t->slot_done[k]) e = hipEventCreateWithFlags(&t->slot_done[k], hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    return pt_fail(PT_EHIP, "%s: staging buffers for %d spheres: %s; the session is as it was", who, cap, hipGetErrorString(e));
  }
  if (t->d_spheres) {
    t->retired_d[t->n_retired] = t->d_spheres, t->retired_h[t->n_retired] = t->h_spheres;
    t->n_retired++;
  }
  t->d_spheres = d, t->h_spheres = h, t->sphere_cap = cap;
  for (bool& used : t->slot_used) used = false;
  t->next_slot = 0;
  return PT_OK;
}

static int ensure_motion_image(const char* who, pt_temporal* t) {
  if (t->d_motion) return PT_OK;
  const hipError_t e = hipMalloc((void**)&t->d_motion, motion_bytes(t));
  if (e == hipSuccess) return PT_OK;
  (void)hipGetLastError();
  t->d_motion = nullptr;
  return pt_fail(PT_EHIP, "%s: the motion image of %zu bytes: %s; the session is as it was", who, motion_bytes(t), hipGetErrorString(e));
}

static int ensure_scene_copy(const char* who, pt_temporal* t, int n) {
  if (n <= t->scene_cap) return PT_OK;
  pt_sphere* s = new (std::nothrow) pt_sphere[n];
  if (!s) return pt_fail(PT_ENOMEM, "%s: out of host memory for the copy of %d spheres", who, n);
  if (t->scene) memcpy(s, t->scene, (size_t)t->scene_n * sizeof(pt_sphere));
  delete[] t->scene;
  t->scene = s, t->scene_cap = n;
  return PT_OK;
}

// The checked spheres through a pinned slot to the device and the motion kernel behind them, on the call's stream.  A slot is
// written again only after the copy out of it has run (with RING slots in flight that wait has normally long passed).
static int launch_motion(pt_temporal* t, const pt_sphere* now, const pt_sphere* prev, int n, const float* B, const float* eye, float4* d_out,
                         hipStream_t s) {
  const int slot = t->next_slot;
  if (t->slot_used[slot]) PT_HIP(hipEventSynchronize(t->slot_done[slot]));
  float4* h = t->h_spheres + (size_t)slot * 2 * t->sphere_cap;
  for (int i = 0; i < n; i++) {
    h[i] = make_float4(now[i].pos[0], now[i].pos[1], now[i].pos[2], now[i].radius);
    h[n + i] = make_float4(prev[i].pos[0], prev[i].pos[1], prev[i].pos[2], prev[i].radius);
  }
  PT_HIP(hipMemcpyAsync(t->d_spheres, h, (size_t)2 * n * sizeof(float4), hipMemcpyHostToDevice, s));
  PT_HIP(hipEventRecord(t->slot_done[slot], s));
  t->slot_used[slot] = true;
  t->next_slot = (slot + 1) % RING;
  MotionParams p{};
  p.width = t->width, p.height = t->height, p.n = n;
  p.fw = (float)t->width, p.fh = (float)t->height;
  for (int k = 0; k < 3; k++) p.b0[k] = B[k], p.e1[k] = B[3 + k] - B[k], p.b2[k] = B[6 + k], p.e2[k] = B[9 + k] - B[6 + k], p.eye[k] = eye[k];
  const dim3 block(BX, BY), grid((unsigned)((p.width + BX - 1) / BX), (unsigned)((p.height + BY - 1) / BY));
  hipLaunchKernelGGL(motion_kernel, grid, block, 0, s, p, (const float4*)t->d_spheres, (const float4*)(t->d_spheres + n), d_out);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// ---- accumulation ---------------------------------------------------------------------------------------------------------

static void session_params(const pt_temporal* t, int samples, Params& p) {
  p.width = t->width, p.height = t->height;
  p.pixels = (uint32_t)t->width * (uint32_t)t->height;
  p.n = (float)samples;
  p.fw = (float)t->width, p.fh = (float)t->height;
  p.cap = t->opts.history_cap, p.depth_tol = t->opts.depth_tol, p.normal_tol = t->opts.normal_tol;
  p.albedo_tol = t->opts.albedo_tol, p.min_weight = t->opts.min_weight;
}

// One frame: the launch and the session's step.  d_motion: null for the static kernel.
static int accumulate_frame(const char* who, pt_temporal* t, Params& p, float* d_frame, const float* B, const float* eye, const float4* d_motion,
                            uint32_t* d_counts, hipStream_t s) {
  for (int k = 0; k < 3; k++) {
    p.b0[k] = B[k], p.e1[k] = B[3 + k] - B[k], p.b2[k] = B[6 + k], p.e2[k] = B[9 + k] - B[6 + k];
    p.eye[k] = eye[k], p.peye[k] = t->eye[k];
  }
  for (int k = 0; k < 9; k++) p.P[k] = t->P[k];
  p.has_history = t->has_history ? 1 : 0;
  float4* hin = t->d_hist + (size_t)t->cur * 3 * p.pixels;
  float4* hout = t->d_hist + (size_t)(1 - t->cur) * 3 * p.pixels;
  const dim3 block(BX, BY), grid((unsigned)((p.width + BX - 1) / BX), (unsigned)((p.height + BY - 1) / BY));
  if (t->antilag.fast_cap > 0.0f) {
    // the FAST form, and behind it -- unless the frame passes through -- the rectify launch on what it wrote
    const float4* fin = t->d_fast + (size_t)t->fcur * p.pixels;
    float4* fout = t->d_fast + (size_t)(1 - t->fcur) * p.pixels;
    const float fast_cap = t->antilag.fast_cap;
    if (d_motion)
      hipLaunchKernelGGL((accumulate_kernel<true, const float4*, const float4*, float4*, float>), grid, block, 0, s, p, d_frame, (const float4*)hin,
                         hout, d_counts, d_motion, fin, fout, fast_cap);
    else
      hipLaunchKernelGGL((accumulate_kernel<false, const float4*, float4*, float>), grid, block, 0, s, p, d_frame, (const float4*)hin, hout,
                         d_counts, fin, fout, fast_cap);
    PT_HIP(hipGetLastError());
    if (p.has_history) {
      RectifyParams rp{p.width, p.height, p.pixels, t->antilag.clamp_sigma};
      switch (t->antilag.clamp_radius) {
        case 1: hipLaunchKernelGGL((rectify_kernel<1>), grid, block, 0, s, rp, d_frame, (const float4*)fout, hout); break;
        case 2: hipLaunchKernelGGL((rectify_kernel<2>), grid, block, 0, s, rp, d_frame, (const float4*)fout, hout); break;
        default: hipLaunchKernelGGL((rectify_kernel<3>), grid, block, 0, s, rp, d_frame, (const float4*)fout, hout); break;
      }
    }
    t->fcur = 1 - t->fcur;
  } else if (d_motion)
    hipLaunchKernelGGL((accumulate_kernel<true, const float4*>), grid, block, 0, s, p, d_frame, (const float4*)hin, hout, d_counts, d_motion);
  else
    hipLaunchKernelGGL((accumulate_kernel<false>), grid, block, 0, s, p, d_frame, (const float4*)hin, hout, d_counts);
  PT_HIP(hipGetLastError());
  (void)camera_matrix(who, B, t->P);  // (checked by the caller)
  for (int k = 0; k < 3; k++) t->eye[k] = eye[k];
  t->cur = 1 - t->cur;
  t->has_history = true;
  return PT_OK;
}

// The calls without a scene; d_motion (single calls only) may be null.  They forget the remembered scene.
static int enqueue_frames(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                          const float* eyes, int samples, const float4* d_motion, uint32_t* d_counts, hipStream_t s) {
  int rc = check_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples);
  if (rc != PT_OK) return rc;
  Params p{};
  session_params(t, samples, p);
  t->has_scene = false;
  for (int f = 0; f < n_frames; f++) {
    // the count image is that of the last frame
    rc = accumulate_frame(who, t, p, d_frames + (size_t)f * frame_stride_floats, bases + 12 * f, eyes + 3 * f, d_motion,
                          f == n_frames - 1 ? d_counts : (uint32_t*)nullptr, s);
    if (rc != PT_OK) return rc;
  }
  return PT_OK;
}

static int run_timed(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                     const float* eyes, int samples, const float4* d_motion, uint32_t* d_counts, float* ms_out) {
  const int rc0 = check_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples);
  if (rc0 != PT_OK) return rc0;
  return pt_stage::run_timed(t->ev0, t->ev1, ms_out, [&] {
    return enqueue_frames(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, d_motion, d_counts, nullptr);
  });
}

// The _scene calls: h_scenes [n_frames][n].  Frame f takes its motion from scene f - 1, the first one from the scene the session
// remembers (none after a reset or a call without a scene: that frame runs the static kernel).
static int check_scene_args(const char* who, const pt_temporal* t, int n_frames, const float* d_frames, size_t frame_stride_floats,
                            const float* bases, const float* eyes, int samples, const pt_sphere* h_scenes, int n) {
  int rc = check_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples);
  if (rc != PT_OK) return rc;
  if (!h_scenes) return pt_fail(PT_EINVAL, "%s: null h_spheres", who);
  if ((rc = check_sphere_count(who, n)) != PT_OK) return rc;
  const bool remembered = t->has_history && t->has_scene;
  if (remembered && n != t->scene_n)
    return pt_fail(PT_EINVAL, "%s: n %d differs from the %d spheres of the session's previous scene: reset the session", who, n, t->scene_n);
  const pt_sphere* prev = remembered ? t->scene : nullptr;
  for (int f = 0; f < n_frames; f++) {
    const pt_sphere* now = h_scenes + (size_t)f * n;
    if ((rc = check_sphere_fields(who, "h_spheres", now, n)) != PT_OK) return rc;
    if (prev && (rc = check_sphere_radii(who, "h_spheres", now, prev, n)) != PT_OK) return rc;
    prev = now;
  }
  return PT_OK;
}

// Every allocation the call needs, before its first launch (and outside a timed window).
static int prepare_scene_call(const char* who, pt_temporal* t, int n_frames, int n) {
  int rc = ensure_scene_copy(who, t, n);
  if (rc == PT_OK && (n_frames > 1 || (t->has_history && t->has_scene))) {
    rc = ensure_motion_image(who, t);
    if (rc == PT_OK) rc = ensure_staging(who, t, n);
  }
  return rc;
}

// The launches of a checked and prepared _scene call.
static int launch_scenes(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                         const float* eyes, int samples, const pt_sphere* h_scenes, int n, uint32_t* d_counts, hipStream_t s) {
  int rc = PT_OK;
  Params p{};
  session_params(t, samples, p);
  for (int f = 0; f < n_frames; f++) {
    const pt_sphere* now = h_scenes + (size_t)f * n;
    const pt_sphere* prev = f ? now - n : (t->has_history && t->has_scene ? t->scene : nullptr);
    const float4* d_motion = nullptr;
    if (t->has_history && prev) {
      if ((rc = launch_motion(t, now, prev, n, bases + 12 * f, eyes + 3 * f, t->d_motion, s)) != PT_OK) return rc;
      d_motion = t->d_motion;
    }
    rc = accumulate_frame(who, t, p, d_frames + (size_t)f * frame_stride_floats, bases + 12 * f, eyes + 3 * f, d_motion,
                          f == n_frames - 1 ? d_counts : (uint32_t*)nullptr, s);
    if (rc != PT_OK) return rc;
    // (the host copy is taken at once: the caller's array need not outlive the call)
    memcpy(t->scene, now, (size_t)n * sizeof(pt_sphere));
    t->scene_n = n, t->has_scene = true;
  }
  return PT_OK;
}

static int enqueue_scenes(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                          const float* eyes, int samples, const pt_sphere* h_scenes, int n, uint32_t* d_counts, hipStream_t s) {
  int rc = check_scene_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n);
  if (rc == PT_OK) rc = prepare_scene_call(who, t, n_frames, n);
  if (rc != PT_OK) return rc;
  return launch_scenes(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n, d_counts, s);
}

static int run_scenes_timed(const char* who, pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                            const float* eyes, int samples, const pt_sphere* h_scenes, int n, uint32_t* d_counts, float* ms_out) {
  int rc = check_scene_args(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n);
  if (rc == PT_OK) rc = prepare_scene_call(who, t, n_frames, n);
  if (rc != PT_OK) return rc;
  return pt_stage::run_timed(t->ev0, t->ev1, ms_out, [&] {
    return launch_scenes(who, t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n, d_counts, nullptr);
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
  if (t->d_motion) (void)hipFree(t->d_motion);
  if (t->d_fast) (void)hipFree(t->d_fast);
  if (t->d_spheres) (void)hipFree(t->d_spheres);
  if (t->h_spheres) (void)hipHostFree(t->h_spheres);
  for (int k = 0; k < t->n_retired; k++) {
    (void)hipFree(t->retired_d[k]);
    (void)hipHostFree(t->retired_h[k]);
  }
  for (hipEvent_t e : t->slot_done)
    if (e) (void)hipEventDestroy(e);
  delete[] t->scene;
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
  const hipError_t e = hipMalloc((void**)&t->d_hist, hist_bytes(t));
  if ((rc = pt_stage::create_events("pt_temporal_create", e, t, pt_temporal_destroy)) != PT_OK) return rc;
  *out = t;
  return PT_OK;
}

int pt_temporal_reset(pt_temporal* t) {
  if (!t) return pt_fail(PT_EINVAL, "pt_temporal_reset: null accumulator");
  t->has_history = false;
  t->has_scene = false;
  return PT_OK;
}

int pt_temporal_workspace_bytes(const pt_temporal* t, uint64_t* bytes) {
  if (!t || !bytes) return pt_fail(PT_EINVAL, "pt_temporal_workspace_bytes: null %s", t ? "output pointer" : "accumulator");
  *bytes = ws_bytes(t);
  return PT_OK;
}

void pt_temporal_antilag_opts_default(pt_temporal_antilag_opts* opts) {
  if (!opts) return;
  *opts = pt_temporal_antilag_opts{};
  opts->fast_cap = 0.0f;
  opts->clamp_sigma = PT_ANTILAG_DEFAULT_SIGMA, opts->clamp_radius = PT_ANTILAG_DEFAULT_RADIUS;
}

int pt_temporal_antilag_check(const pt_temporal_antilag_opts* opts, float history_cap) {
  return check_antilag("pt_temporal_antilag_check", opts, history_cap);
}

int pt_temporal_set_antilag(pt_temporal* t, const pt_temporal_antilag_opts* opts) {
  const char* who = "pt_temporal_set_antilag";
  if (!t) return pt_fail(PT_EINVAL, "%s: null accumulator", who);
  const int rc = check_antilag(who, opts, t->opts.history_cap);
  if (rc != PT_OK) return rc;
  if (t->has_history) return pt_fail(PT_EINVAL, "%s: the session holds a history: reset the session", who);
  if (opts->fast_cap > 0.0f && !t->d_fast) {
    const hipError_t e = hipMalloc((void**)&t->d_fast, fast_bytes(t));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      t->d_fast = nullptr;
      return pt_fail(PT_EHIP, "%s: the fast images of %zu bytes: %s; the session is as it was", who, fast_bytes(t), hipGetErrorString(e));
    }
  }
  t->antilag = *opts;
  return PT_OK;
}

int pt_temporal_fast(pt_temporal* t, float* d_out, void* hip_stream) {
  const char* who = "pt_temporal_fast";
  if (!t || !d_out) return pt_fail(PT_EINVAL, "%s: null %s", who, t ? "d_out" : "accumulator");
  if (!(t->antilag.fast_cap > 0.0f)) return pt_fail(PT_EINVAL, "%s: anti-lag is off (pt_temporal_set_antilag, fast_cap > 0)", who);
  if (!t->has_history) return pt_fail(PT_EINVAL, "%s: no frame has run since the session was made or reset", who);
  const size_t pixels = (size_t)t->width * t->height;
  PT_HIP(hipMemcpyAsync(d_out, t->d_fast + (size_t)t->fcur * pixels, pixels * sizeof(float4), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return PT_OK;
}

int pt_temporal_enqueue(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                        void* hip_stream) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_enqueue: null %s", t ? "d_frame" : "accumulator");
  return enqueue_frames("pt_temporal_enqueue", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, nullptr, d_counts,
                        (hipStream_t)hip_stream);
}

int pt_temporal_run(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                    float* ms_out) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_run: null %s", t ? "d_frame" : "accumulator");
  return run_timed("pt_temporal_run", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, nullptr, d_counts, ms_out);
}

int pt_temporal_enqueue_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                               const float* eyes, int samples, uint32_t* d_counts, void* hip_stream) {
  return enqueue_frames("pt_temporal_enqueue_frames", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, nullptr, d_counts,
                        (hipStream_t)hip_stream);
}

int pt_temporal_run_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                           const float* eyes, int samples, uint32_t* d_counts, float* ms_out) {
  return run_timed("pt_temporal_run_frames", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, nullptr, d_counts, ms_out);
}

int pt_temporal_scene_check(const pt_sphere* h_now, const pt_sphere* h_prev, int n, const float basis[12], const float eye[3]) {
  return check_motion_args("pt_temporal_scene_check", h_now, h_prev, n, basis, eye);
}

int pt_temporal_motion(pt_temporal* t, const pt_sphere* h_now, const pt_sphere* h_prev, int n, const float basis[12], const float eye[3],
                       float* d_motion, void* hip_stream) {
  const char* who = "pt_temporal_motion";
  if (!t) return pt_fail(PT_EINVAL, "%s: null accumulator", who);
  if (!d_motion) return pt_fail(PT_EINVAL, "%s: null d_motion", who);
  int rc = check_motion_args(who, h_now, h_prev, n, basis, eye);
  if (rc == PT_OK) rc = ensure_staging(who, t, n);
  if (rc != PT_OK) return rc;
  return launch_motion(t, h_now, h_prev, n, basis, eye, (float4*)d_motion, (hipStream_t)hip_stream);
}

int pt_temporal_enqueue_motion(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const float* d_motion,
                               uint32_t* d_counts, void* hip_stream) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_enqueue_motion: null %s", t ? "d_frame" : "accumulator");
  return enqueue_frames("pt_temporal_enqueue_motion", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples,
                        (const float4*)d_motion, d_counts, (hipStream_t)hip_stream);
}

int pt_temporal_run_motion(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const float* d_motion,
                           uint32_t* d_counts, float* ms_out) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_run_motion: null %s", t ? "d_frame" : "accumulator");
  return run_timed("pt_temporal_run_motion", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, (const float4*)d_motion,
                   d_counts, ms_out);
}

int pt_temporal_enqueue_scene(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const pt_sphere* h_spheres,
                              int n, uint32_t* d_counts, void* hip_stream) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_enqueue_scene: null %s", t ? "d_frame" : "accumulator");
  return enqueue_scenes("pt_temporal_enqueue_scene", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, h_spheres, n,
                        d_counts, (hipStream_t)hip_stream);
}

int pt_temporal_run_scene(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const pt_sphere* h_spheres,
                          int n, uint32_t* d_counts, float* ms_out) {
  if (!t || !d_frame) return pt_fail(PT_EINVAL, "pt_temporal_run_scene: null %s", t ? "d_frame" : "accumulator");
  return run_scenes_timed("pt_temporal_run_scene", t, 1, d_frame, (size_t)t->width * t->height * 14, basis, eye, samples, h_spheres, n,
                          d_counts, ms_out);
}

int pt_temporal_enqueue_frames_scenes(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                                      const float* eyes, const pt_sphere* h_scenes, int n, int samples, uint32_t* d_counts, void* hip_stream) {
  return enqueue_scenes("pt_temporal_enqueue_frames_scenes", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n,
                        d_counts, (hipStream_t)hip_stream);
}

int pt_temporal_run_frames_scenes(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                                  const float* eyes, const pt_sphere* h_scenes, int n, int samples, uint32_t* d_counts, float* ms_out) {
  return run_scenes_timed("pt_temporal_run_frames_scenes", t, n_frames, d_frames, frame_stride_floats, bases, eyes, samples, h_scenes, n,
                          d_counts, ms_out);
}

}  // extern "C"
