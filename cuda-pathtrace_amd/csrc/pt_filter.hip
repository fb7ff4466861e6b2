// pt_filter.hip -- the weights-free denoiser behind pt_filter_* (include/ptcore.h): an edge-avoiding a-trous wavelet filter
// on albedo-demodulated colour whose luminance stop is scaled by the pixel's own variance (the spatial stage of SVGF) and
// whose stops on normal, albedo and depth come from the frame's own channels (src/pathtrace.cu:240-254 writes all 14).
// No counterpart in the reference.  DENOISER.md, "Feature-guided filter", states the definition; tests/filter_model.py
// restates it in NumPy.  TOLERANCED code like pt_fast.hip: FMA contraction in the tap loop, hardware exp2 / rcp.
//
// Three kernels, one lane per pixel, blockIdx.z = frame of the group:
//   prepare  frame -> state {ill.rgb, var} and the guides {n.xyz, z}, {alb.rgb, dz}: three float4 per pixel
//   spatial  only with pt_filter_set_spatial: var <- fmax(var, spread of the (2R+1)^2 neighbours' luminances on the pixel's
//            surface) for the pixels with fewer than `below` samples, window from LDS, state A -> state B
//   atrous   25 taps at a run-time step (TILE 1, 2: at that step from LDS), state ping-pong; the LAST iteration multiplies the albedo back and writes the
//            caller's frame (or d_rgb), so no iteration ever reads the caller's frame and in-place use is safe.
// Per tap: three 16-byte loads, one sum of the four stops, ONE exp2.  Per pixel: the reciprocals of the luminance stop and of
// the depth stop's five distinct tap distances.  Steps 1 and 2 read an LDS tile of the workgroup's pixels and their halo, the
// larger steps load directly (DENOISER.md, "Speed": the tile makes those two launches 1.7 times faster).  The lab library's
// pt_debug_filter_state runs unfused iterations and copies the state and the guides out; tests/test_filter_exact_gpu.py holds
// the set-up, every stop and var' to the bit with it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "pt_stage.h"
#if PT_BUILD_EXPERIMENTS
#include "../../include/ptcore_lab.h"
#endif

namespace ptflt {

constexpr float EPS = 0.00316f;  // train.py:48-55's pre-processing constant, as in pt_denoise.hip
constexpr int BX = 32, BY = 8;   // workgroup: 32 columns x 8 rows, a wave covers two rows of 32 pixels

struct Params {
  int width, height;
  uint32_t pixels;       // width x height
  size_t frame_stride;   // floats between the caller's frames
  size_t out_stride;     // floats between the output frames
  int out_ld;            // 14 (in place) or 3 (d_rgb)
  float cn, ca;          // log2(e) / sigma_n^2, log2(e) / sigma_a^2
  float sz, sl;          // sigma_z, sigma_l
  float samples;         // uniform count (unused with a count image)
};

#pragma clang fp contract(off)

__device__ __forceinline__ float lum(float x, float y, float z) { return 0.2126f * x + 0.7152f * y + 0.0722f * z; }

// s + w x and s + w (d d), every operation rounded: the moments of spatial_kernel
__device__ __forceinline__ float add_weighted(float s, float w, float x) { return s + w * x; }
__device__ __forceinline__ float add_weighted_square(float s, float w, float d) { return s + w * (d * d); }

// Set-up.  Rounded operation by operation like the float32 NumPy twin (divisions are IEEE).
__global__ void __launch_bounds__(BX* BY) prepare_kernel(Params p, const float* __restrict__ frames, const uint32_t* __restrict__ counts,
                                                         float4* __restrict__ state, float4* __restrict__ g0, float4* __restrict__ g1) {
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  if (x >= p.width || y >= p.height) return;
  const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
  const float* frame = frames + (size_t)blockIdx.z * p.frame_stride;
  const float* px = frame + (size_t)i * 14;
  const float ax = EPS + px[6], ay = EPS + px[7], az = EPS + px[8];
  const float ix = px[0] / ax, iy = px[1] / ay, iz = px[2] / az;
  const float n = counts ? (float)counts[i] : p.samples;
  float var;
  if (n >= 2.0f) {
    const float la = lum(ax, ay, az);
    var = px[10] / n / (la * la);
  } else {
    const float li = lum(ix, iy, iz);
    var = li * li;
  }
  const int xl = x > 0 ? x - 1 : 0, xr = x < p.width - 1 ? x + 1 : x;
  const int yu = y > 0 ? y - 1 : 0, yd = y < p.height - 1 ? y + 1 : y;
  const size_t row = (size_t)y * p.width, col = (size_t)x;
  const float dzx = fabsf(frame[(row + xr) * 14 + 9] - frame[(row + xl) * 14 + 9]);
  const float dzy = fabsf(frame[((size_t)yd * p.width + col) * 14 + 9] - frame[((size_t)yu * p.width + col) * 14 + 9]);
  const size_t o = (size_t)blockIdx.z * p.pixels + i;
  state[o] = make_float4(ix, iy, iz, var);
  g0[o] = make_float4(px[3], px[4], px[5], px[9]);
  g1[o] = make_float4(px[6], px[7], px[8], 0.5f * fmaxf(dzx, dzy));
}

#pragma clang fp contract(fast)

// One iteration at `step`.  FUSED: the last one -- writes (ill' x (EPS + albedo)) to `out` instead of the next state.
// TILE = 0: every tap is a global load.  TILE = 1 or 2 (step == TILE): the workgroup first copies its 32 x 8 pixels and a halo
// of 2 x TILE, clamped to the frame, of all three images into LDS and the taps and the blur read that tile.  The arithmetic is
// the same expression on the same values in the same order, so the two forms give the same bits.
template <bool FUSED, int TILE>
__global__ void __launch_bounds__(BX* BY) atrous_kernel(Params p, int step, const float4* __restrict__ src, const float4* __restrict__ g0,
                                                        const float4* __restrict__ g1, float4* __restrict__ dst, float* __restrict__ out) {
  constexpr int HALO = 2 * TILE, TW = BX + 2 * HALO, TH = BY + 2 * HALO;
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  const size_t base = (size_t)blockIdx.z * p.pixels;
  src += base, g0 += base, g1 += base;
  const uint32_t W = (uint32_t)p.width;
  const float4 *ts = nullptr, *tn = nullptr, *ta = nullptr;  // the tile's images
  if constexpr (TILE > 0) {
    __shared__ float4 tile[3][TH * TW];
    const int x0 = (int)(blockIdx.x * BX) - HALO, y0 = (int)(blockIdx.y * BY) - HALO;
    for (int t = threadIdx.y * BX + threadIdx.x; t < TH * TW; t += BX * BY) {
      const int gx = min(max(x0 + t % TW, 0), p.width - 1), gy = min(max(y0 + t / TW, 0), p.height - 1);
      const uint32_t q = (uint32_t)gy * W + (uint32_t)gx;
      tile[0][t] = src[q], tile[1][t] = g0[q], tile[2][t] = g1[q];
    }
    __syncthreads();
    ts = tile[0], tn = tile[1], ta = tile[2];
  }
  if (x >= p.width || y >= p.height) return;
  const uint32_t i = (uint32_t)y * W + (uint32_t)x;
  const int ti = (threadIdx.y + HALO) * TW + threadIdx.x + HALO;  // this pixel in the tile
  const float4 sp = TILE ? ts[ti] : src[i], np = TILE ? tn[ti] : g0[i], ap = TILE ? ta[ti] : g1[i];

  // 3 x 3 (1/4, 1/2, 1/4)^2 blur of the variance, replicated edges (the tile's halo is clamped, so it replicates them too)
  const uint32_t xl = x > 0 ? x - 1 : 0, xr = x < p.width - 1 ? x + 1 : x;
  const uint32_t rows[3] = {(uint32_t)(y > 0 ? y - 1 : 0) * W, (uint32_t)y * W, (uint32_t)(y < p.height - 1 ? y + 1 : y) * W};
  float g = 0.0f;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float k = r == 1 ? 0.5f : 0.25f;
    const int tr = ti + (r - 1) * TW;
    const float vl = TILE ? ts[tr - 1].w : src[rows[r] + xl].w, vc = TILE ? ts[tr].w : src[rows[r] + x].w;
    const float vr = TILE ? ts[tr + 1].w : src[rows[r] + xr].w;
    g += k * (0.25f * vl + 0.5f * vc + 0.25f * vr);
  }
  const float sd = __builtin_sqrtf(fmaxf(g, 0.0f));
  const float Lp = lum(sp.x, sp.y, sp.z);
  constexpr float LOG2E = 1.4426950408889634f;
  const float rl = LOG2E * __builtin_amdgcn_rcpf(p.sl * sd + 0.01f * fabsf(Lp) + 1e-4f);
  // depth stop: sigma_z dz d + 1e-3 |z| + 1e-20 for d = step x sqrt(i^2 + j^2), i^2 + j^2 in {1, 2, 4, 5, 8}
  const float zs = p.sz * ap.w * (float)step, zc = 1e-3f * fabsf(np.w) + 1e-20f;
  float rz[9];
  rz[0] = 0.0f;  // the centre: |z_q - z_p| is 0
  rz[1] = LOG2E * __builtin_amdgcn_rcpf(zs + zc);
  rz[2] = LOG2E * __builtin_amdgcn_rcpf(zs * 1.41421356237309505f + zc);
  rz[4] = LOG2E * __builtin_amdgcn_rcpf(zs * 2.0f + zc);
  rz[5] = LOG2E * __builtin_amdgcn_rcpf(zs * 2.23606797749978970f + zc);
  rz[8] = LOG2E * __builtin_amdgcn_rcpf(zs * 2.82842712474619010f + zc);
  rz[3] = rz[6] = rz[7] = 0.0f;  // (no tap has these)

  float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
#pragma unroll
  for (int j = -2; j <= 2; j++) {
    const int qy = y + j * step;
    const bool rowin = qy >= 0 && qy < p.height;
    const uint32_t qrow = rowin ? (uint32_t)qy * W : (uint32_t)y * W;
#pragma unroll
    for (int k = -2; k <= 2; k++) {
      const int qx = x + k * step;
      const bool in = rowin && qx >= 0 && qx < p.width;
      // a tap outside the frame is skipped: it reads a pixel inside the frame instead (the pixel's own row / column, in both
      // forms: one of its own taps, so a non-finite pixel reaches the same outputs through the tile and through direct loads)
      // and gets weight 0
      const uint32_t q = qrow + (uint32_t)(qx >= 0 && qx < p.width ? qx : x);
      const int tq = ti + (rowin ? j : 0) * TILE * TW + (qx >= 0 && qx < p.width ? k : 0) * TILE;
      const float4 sq = TILE ? ts[tq] : src[q], nq = TILE ? tn[tq] : g0[q], aq = TILE ? ta[tq] : g1[q];
      const float kj = j == 0 ? 0.375f : (j == 1 || j == -1) ? 0.25f : 0.0625f;
      const float kk = k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f;
      const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
      const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
      const float Lq = lum(sq.x, sq.y, sq.z);
      float e = (dnx * dnx + dny * dny + dnz * dnz) * p.cn + (dax * dax + day * day + daz * daz) * p.ca;
      e += fabsf(nq.w - np.w) * rz[j * j + k * k];
      e += fabsf(Lq - Lp) * rl;
      const float w = in ? (kj * kk) * __builtin_amdgcn_exp2f(-e) : 0.0f;
      sw += w;
      sx += w * sq.x, sy += w * sq.y, sz += w * sq.z;
      sv += (w * w) * sq.w;
    }
  }
  const float ox = sx / sw, oy = sy / sw, oz = sz / sw;  // IEEE divisions: sw >= 9/64 (the centre tap)
  if (FUSED) {
    float* o = out + (size_t)blockIdx.z * p.out_stride + (size_t)i * p.out_ld;
    o[0] = ox * (EPS + ap.x), o[1] = oy * (EPS + ap.y), o[2] = oz * (EPS + ap.z);
  } else {
    dst[base + i] = make_float4(ox, oy, oz, sv / (sw * sw));
  }
}
// The spatial variance estimate (DENOISER.md, "Spatial variance estimate"; tests/filter_spatial_model.py), between the set-up and
// the first iteration: a pixel with fewer than `below` samples takes var <- fmax(var, v), v the weighted variance of L = lum(ill)
// over the (2R+1)^2 window, weighted by the normal, albedo and depth stops of the iterations (step 1, no luminance stop, no
// a-trous kernel).  Reads state A and the guides, writes the whole state {ill, new var} to state B: no lane stores into an image
// another lane loads.  The workgroup stages what the taps need -- {n.xyz, z} and {alb.rgb, L} -- for its pixels and a halo of R,
// clamped to the frame, as two planes of 16-byte entries: the lanes of a row read consecutive entries, which is conflict-free
// for ds_read_b128 whatever the row length (a wave's second row is the other half-wave), where one 32-byte entry per pixel would
// put lanes l and l + 8 of a group on one bank.  R = 3: 2 x 14 x 38 x 16 = 17024 bytes.
// Contraction: this kernel lies in the file's contract(fast) region, so the exponent e may contract (toleranced: hardware exp2 /
// rcp, log2(e) folded into the stop factors).  The two moment passes go through add_weighted / add_weighted_square, defined in
// the contract(off) region above, row by row through the window, and m and v are IEEE quotients: with weights of exactly 0 or 1
// they are the float32 model's bits.
template <int R>
__global__ void __launch_bounds__(BX* BY) spatial_kernel(Params p, uint32_t below, uint32_t samples, const uint32_t* __restrict__ counts,
                                                         const float4* __restrict__ src, const float4* __restrict__ g0,
                                                         const float4* __restrict__ g1, float4* __restrict__ dst) {
  constexpr int TW = BX + 2 * R, TH = BY + 2 * R, D = 2 * R + 1;
  __shared__ float4 tile[2][TH * TW];
  const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
  const size_t base = (size_t)blockIdx.z * p.pixels;
  src += base, g0 += base, g1 += base;
  const uint32_t W = (uint32_t)p.width;
  const int x0 = (int)(blockIdx.x * BX) - R, y0 = (int)(blockIdx.y * BY) - R;
  for (int t = threadIdx.y * BX + threadIdx.x; t < TH * TW; t += BX * BY) {
    const int gx = min(max(x0 + t % TW, 0), p.width - 1), gy = min(max(y0 + t / TW, 0), p.height - 1);
    const uint32_t q = (uint32_t)gy * W + (uint32_t)gx;
    const float4 s = src[q], a = g1[q];
    tile[0][t] = g0[q], tile[1][t] = make_float4(a.x, a.y, a.z, lum(s.x, s.y, s.z));
  }
  __syncthreads();
  if (x >= p.width || y >= p.height) return;
  const uint32_t i = (uint32_t)y * W + (uint32_t)x;
  const float4 sp = src[i];
  const uint32_t n = counts ? counts[i] : samples;
  if (n >= below) {  // enough samples: the set-up's state bit for bit
    dst[base + i] = sp;
    return;
  }
  const float4 *tn = tile[0], *ta = tile[1];
  const int ti = (threadIdx.y + R) * TW + threadIdx.x + R;  // this pixel in the tile
  const float4 np = tn[ti], ap = ta[ti];
  constexpr float LOG2E = 1.4426950408889634f;
  // depth stop: sigma_z dz d + 1e-3 |z| + 1e-20 for d = sqrt(i^2 + j^2), i^2 + j^2 in {1, 2, 4, 5, 8, 9, 10, 13, 18}
  constexpr float ROOT[19] = {0.0f, 1.0f, 1.41421356237309505f, 0.0f, 2.0f, 2.23606797749978970f, 0.0f, 0.0f, 2.82842712474619010f, 3.0f,
                              3.16227766016837933f, 0.0f, 0.0f, 3.60555127546398929f, 0.0f, 0.0f, 0.0f, 0.0f, 4.24264068711928515f};
  const float zs = p.sz * g1[i].w, zc = 1e-3f * fabsf(np.w) + 1e-20f;
  float rz[2 * R * R + 1];
  rz[0] = 0.0f;
#pragma unroll
  for (int d2 = 1; d2 <= 2 * R * R; d2++) rz[d2] = ROOT[d2] != 0.0f ? LOG2E * __builtin_amdgcn_rcpf(zs * ROOT[d2] + zc) : 0.0f;

  float w[D * D];
  float sw = 0.0f, sl = 0.0f;
#pragma unroll
  for (int j = -R; j <= R; j++) {
    const bool rowin = y + j >= 0 && y + j < p.height;
#pragma unroll
    for (int k = -R; k <= R; k++) {
      const bool colin = x + k >= 0 && x + k < p.width;
      // a tap outside the frame is skipped: it reads the pixel's own row / column instead, one of its own taps, at weight 0
      const int tq = ti + (rowin ? j : 0) * TW + (colin ? k : 0);
      const float4 nq = tn[tq], aq = ta[tq];
      const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
      const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
      float e = (dnx * dnx + dny * dny + dnz * dnz) * p.cn + (dax * dax + day * day + daz * daz) * p.ca;
      e += fabsf(nq.w - np.w) * rz[j * j + k * k];
      const float wq = rowin && colin ? (j == 0 && k == 0 ? 1.0f : __builtin_amdgcn_exp2f(-e)) : 0.0f;
      w[(j + R) * D + k + R] = wq;
      sw = add_weighted(sw, wq, 1.0f);
      sl = add_weighted(sl, wq, aq.w - ap.w);  // relative to the pixel's own L: the same v, and exactly 0 on a flat window
    }
  }
  const float m = sl / sw;  // the mean of L_q - L_p.  IEEE divisions: sw >= 1 (the centre tap)
  float sv = 0.0f;
#pragma unroll
  for (int j = -R; j <= R; j++) {
    const bool rowin = y + j >= 0 && y + j < p.height;
#pragma unroll
    for (int k = -R; k <= R; k++) {
      const bool colin = x + k >= 0 && x + k < p.width;
      const int tq = ti + (rowin ? j : 0) * TW + (colin ? k : 0);
      sv = add_weighted_square(sv, w[(j + R) * D + k + R], (ta[tq].w - ap.w) - m);
    }
  }
  dst[base + i] = make_float4(sp.x, sp.y, sp.z, fmaxf(sp.w, sv / sw));  // fmax: a NaN v leaves var as it was
}
}  // namespace ptflt

using namespace ptflt;

struct pt_filter {
  int width = 0, height = 0;
  pt_filter_opts opts{};
  int max_frames = 1;
  bool tiled = true;  // steps 1 and 2 through the LDS tile (the lab library's pt_debug_filter_tiled switches it off for the A/B)
  pt_filter_spatial_opts spatial{};  // below 0: off (pt_filter_set_spatial)
  float4* d_ws = nullptr;  // [4][max_frames x pixels]: state A, state B, guide 0, guide 1
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static size_t ws_bytes(const pt_filter* f, int frames) { return (size_t)4 * frames * f->width * f->height * sizeof(float4); }

static Params make_params(const pt_filter* f, size_t frame_stride, size_t out_stride, int out_ld, int samples) {
  Params p{};
  p.width = f->width, p.height = f->height;
  p.pixels = (uint32_t)f->width * (uint32_t)f->height;
  p.frame_stride = frame_stride, p.out_stride = out_stride, p.out_ld = out_ld;
  // clamped to the largest float: a sigma below about 6.6e-20 is a hard stop (0 stays 0, any difference is refused), where an
  // infinite factor would make the centre tap's 0 x inf a NaN
  const double log2e = 1.4426950408889634, flt_max = 3.4028234663852886e38;
  p.cn = (float)fmin(log2e / ((double)f->opts.sigma_n * (double)f->opts.sigma_n), flt_max);
  p.ca = (float)fmin(log2e / ((double)f->opts.sigma_a * (double)f->opts.sigma_a), flt_max);
  p.sz = f->opts.sigma_z, p.sl = f->opts.sigma_l;
  p.samples = (float)samples;
  return p;
}

// One group of g <= max_frames frames: prepare, the spatial variance estimate if it is on and a pixel can qualify (a count image,
// or the uniform `samples` below the threshold), then the iterations (steps[0 .. n_steps)), the last one fused.  With `state`
// (the lab library's pt_debug_filter_state) no iteration is fused, nothing is written to `out`, and *state receives the
// workspace image that holds the state after the last iteration.
static int launch_group(const pt_filter* f, const Params& p, int g, const float* frames, float* out, const uint32_t* counts, int samples,
                        const int* steps, int n_steps, hipStream_t s, const float4** state = nullptr) {
  const size_t n = (size_t)f->max_frames * p.pixels;
  float4 *a = f->d_ws, *b = f->d_ws + n, *g0 = f->d_ws + 2 * n, *g1 = f->d_ws + 3 * n;
  const dim3 block(BX, BY), grid((unsigned)((p.width + BX - 1) / BX), (unsigned)((p.height + BY - 1) / BY), (unsigned)g);
  hipLaunchKernelGGL(prepare_kernel, grid, block, 0, s, p, frames, counts, a, g0, g1);
  const uint32_t below = f->spatial.below;
  if (below > 0 && (counts || (uint32_t)samples < below)) {
    using Spatial = void (*)(Params, uint32_t, uint32_t, const uint32_t*, const float4*, const float4*, const float4*, float4*);
    static const Spatial spatial[3] = {spatial_kernel<1>, spatial_kernel<2>, spatial_kernel<3>};
    hipLaunchKernelGGL(spatial[f->spatial.radius - 1], grid, block, 0, s, p, below, (uint32_t)samples, counts, (const float4*)a,
                       (const float4*)g0, (const float4*)g1, b);
    float4* t = a;
    a = b, b = t;
  }
  using Kernel = void (*)(Params, int, const float4*, const float4*, const float4*, float4*, float*);
  static const Kernel kernels[2][3] = {{atrous_kernel<false, 0>, atrous_kernel<false, 1>, atrous_kernel<false, 2>},
                                       {atrous_kernel<true, 0>, atrous_kernel<true, 1>, atrous_kernel<true, 2>}};
  for (int k = 0; k < n_steps; k++) {
    const int tile = f->tiled && steps[k] <= 2 ? steps[k] : 0;
    if (k == n_steps - 1 && !state) {
      hipLaunchKernelGGL(kernels[1][tile], grid, block, 0, s, p, steps[k], (const float4*)a, (const float4*)g0, (const float4*)g1,
                         (float4*)nullptr, out);
    } else {
      hipLaunchKernelGGL(kernels[0][tile], grid, block, 0, s, p, steps[k], (const float4*)a, (const float4*)g0, (const float4*)g1, b,
                         (float*)nullptr);
      float4* t = a;
      a = b, b = t;
    }
  }
  if (state) *state = a;
  PT_HIP(hipGetLastError());
  return PT_OK;
}

static int check_frames_args(const char* who, const pt_filter* f, int n_frames, const float* d_frames, size_t frame_stride_floats,
                             const float* d_rgb, size_t rgb_stride_floats, int samples, const uint32_t* d_counts) {
  if (!f) return pt_fail(PT_EINVAL, "%s: null filter", who);
  if (!d_frames) return pt_fail(PT_EINVAL, "%s: null d_frames", who);
  if (n_frames < 1) return pt_fail(PT_EINVAL, "%s: n_frames %d < 1", who, n_frames);
  const size_t pixels = (size_t)f->width * f->height;
  if (frame_stride_floats < pixels * 14)
    return pt_fail(PT_EINVAL, "%s: frame_stride_floats %zu < width x height x 14 = %zu", who, frame_stride_floats, pixels * 14);
  if (d_rgb && rgb_stride_floats < pixels * 3)
    return pt_fail(PT_EINVAL, "%s: rgb_stride_floats %zu < width x height x 3 = %zu", who, rgb_stride_floats, pixels * 3);
  if (!d_counts && samples < 1) return pt_fail(PT_EINVAL, "%s: samples %d < 1 (and no count image)", who, samples);
  return PT_OK;
}

static int enqueue_frames(const char* who, pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                          size_t rgb_stride_floats, int samples, const uint32_t* d_counts, hipStream_t s) {
  int rc = check_frames_args(who, f, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, samples, d_counts);
  if (rc != PT_OK) return rc;
  const Params p = make_params(f, frame_stride_floats, d_rgb ? rgb_stride_floats : frame_stride_floats, d_rgb ? 3 : 14, samples);
  int steps[8];
  for (int k = 0; k < f->opts.iterations; k++) steps[k] = 1 << k;
  for (int f0 = 0; f0 < n_frames; f0 += f->max_frames) {
    const int g = n_frames - f0 < f->max_frames ? n_frames - f0 : f->max_frames;
    float* frames = d_frames + (size_t)f0 * frame_stride_floats;
    float* out = d_rgb ? d_rgb + (size_t)f0 * rgb_stride_floats : frames;
    if ((rc = launch_group(f, p, g, frames, out, d_counts, samples, steps, f->opts.iterations, s)) != PT_OK) return rc;
  }
  return PT_OK;
}

extern "C" {

void pt_filter_opts_default(pt_filter_opts* opts) {
  if (!opts) return;
  *opts = pt_filter_opts{};
  opts->iterations = 5;
  opts->sigma_l = 4.0f, opts->sigma_n = 0.35f, opts->sigma_a = 0.1f, opts->sigma_z = 1.0f;
  opts->max_frames = 1;
}

void pt_filter_spatial_opts_default(pt_filter_spatial_opts* opts) {
  if (!opts) return;
  *opts = pt_filter_spatial_opts{};
  opts->radius = PT_FILTER_SPATIAL_DEFAULT_RADIUS;
}

static int spatial_check(const char* who, const pt_filter_spatial_opts* opts) {
  if (!opts) return pt_fail(PT_EINVAL, "%s: null opts", who);
  if (opts->radius < 1 || opts->radius > 3) return pt_fail(PT_EINVAL, "%s: radius %d outside 1 .. 3", who, opts->radius);
  for (int i = 0; i < 2; i++)
    if (opts->reserved[i] != 0) return pt_fail(PT_EINVAL, "%s: reserved[%d] = %d must be 0", who, i, opts->reserved[i]);
  return PT_OK;
}

int pt_filter_spatial_check(const pt_filter_spatial_opts* opts) { return spatial_check("pt_filter_spatial_check", opts); }

int pt_filter_set_spatial(pt_filter* f, const pt_filter_spatial_opts* opts) {
  pt_filter_spatial_opts o;
  pt_filter_spatial_opts_default(&o);  // NULL: off
  if (opts) {  // (the options first: a bad one is refused whatever the filter)
    const int rc = spatial_check("pt_filter_set_spatial", opts);
    if (rc != PT_OK) return rc;
    o = *opts;
  }
  if (!f) return pt_fail(PT_EINVAL, "pt_filter_set_spatial: null filter");
  f->spatial = o;
  return PT_OK;
}

int pt_filter_destroy(pt_filter* f) {
  if (!f) return PT_OK;
  if (f->d_ws) (void)hipFree(f->d_ws);
  pt_stage::destroy_events(f);
  delete f;
  return PT_OK;
}

int pt_filter_create(int width, int height, const pt_filter_opts* opts, pt_filter** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_filter_create: null output pointer");
  *out = nullptr;
  pt_filter_opts o;
  if (opts) o = *opts;
  else pt_filter_opts_default(&o);
  int rc = pt_stage::check_frame_size("pt_filter_create", width, height);
  if (rc != PT_OK) return rc;
  if (o.iterations < 1 || o.iterations > 8) return pt_fail(PT_EINVAL, "pt_filter_create: iterations %d outside 1 .. 8", o.iterations);
  const struct { const char* name; float v; } sig[4] = {{"sigma_l", o.sigma_l}, {"sigma_n", o.sigma_n}, {"sigma_a", o.sigma_a}, {"sigma_z", o.sigma_z}};
  for (const auto& s : sig)
    if (!(s.v > 0.0f) || !(s.v <= 3.4028234663852886e38f))
      return pt_fail(PT_EINVAL, "pt_filter_create: %s %g must be finite and > 0", s.name, (double)s.v);
  if (o.max_frames < 1) return pt_fail(PT_EINVAL, "pt_filter_create: max_frames %d < 1", o.max_frames);
  if ((rc = pt_stage::check_batch("pt_filter_create", o.max_frames, width, height)) != PT_OK) return rc;
  for (int i = 0; i < 2; i++)
    if (o.reserved[i] != 0) return pt_fail(PT_EINVAL, "pt_filter_create: reserved[%d] = %d must be 0", i, o.reserved[i]);
  if ((rc = pt_stage::check_device("pt_filter_create")) != PT_OK) return rc;
  pt_filter* f = new (std::nothrow) pt_filter();
  if (!f) return pt_fail(PT_ENOMEM, "pt_filter_create: out of host memory");
  f->width = width, f->height = height, f->opts = o, f->max_frames = o.max_frames;
  const hipError_t e = hipMalloc((void**)&f->d_ws, ws_bytes(f, f->max_frames));
  if ((rc = pt_stage::create_events("pt_filter_create", e, f, pt_filter_destroy)) != PT_OK) return rc;
  *out = f;
  return PT_OK;
}

int pt_filter_reserve_frames(pt_filter* f, int max_frames) {
  if (!f) return pt_fail(PT_EINVAL, "pt_filter_reserve_frames: null filter");
  if (max_frames < 1) return pt_fail(PT_EINVAL, "pt_filter_reserve_frames: max_frames %d < 1", max_frames);
  if (max_frames <= f->max_frames) return PT_OK;
  int rc = pt_stage::check_batch("pt_filter_reserve_frames", max_frames, f->width, f->height);
  if (rc != PT_OK) return rc;
  const pt_stage::Buffer bufs[1] = {{(void**)&f->d_ws, ws_bytes(f, max_frames), false}};
  rc = pt_stage::grow_workspace("pt_filter_reserve_frames", bufs, "%d frames (%zu bytes)", max_frames, ws_bytes(f, max_frames));
  if (rc != PT_OK) return rc;
  f->max_frames = max_frames;
  return PT_OK;
}

int pt_filter_workspace_bytes(const pt_filter* f, uint64_t* bytes) {
  if (!f || !bytes) return pt_fail(PT_EINVAL, "pt_filter_workspace_bytes: null %s", f ? "output pointer" : "filter");
  *bytes = ws_bytes(f, f->max_frames);
  return PT_OK;
}

int pt_filter_enqueue_frames(pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                             size_t rgb_stride_floats, int samples, void* hip_stream) {
  return enqueue_frames("pt_filter_enqueue_frames", f, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, samples, nullptr,
                        (hipStream_t)hip_stream);
}

int pt_filter_enqueue(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, void* hip_stream) {
  if (!f || !d_frame) return pt_fail(PT_EINVAL, "pt_filter_enqueue: null %s", f ? "d_frame" : "filter");
  const size_t pixels = (size_t)f->width * f->height;
  return enqueue_frames("pt_filter_enqueue", f, 1, d_frame, pixels * 14, d_rgb, pixels * 3, samples, d_counts, (hipStream_t)hip_stream);
}

static int run_timed(const char* who, pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                     size_t rgb_stride_floats, int samples, const uint32_t* d_counts, float* ms_out) {
  // (arguments first: a refused call must not touch the device)
  const int rc0 = check_frames_args(who, f, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, samples, d_counts);
  if (rc0 != PT_OK) return rc0;
  return pt_stage::run_timed(f->ev0, f->ev1, ms_out, [&] {
    return enqueue_frames(who, f, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, samples, d_counts, nullptr);
  });
}

int pt_filter_run_frames(pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb, size_t rgb_stride_floats,
                         int samples, float* ms_out) {
  return run_timed("pt_filter_run_frames", f, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, samples, nullptr, ms_out);
}

int pt_filter_run(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, float* ms_out) {
  if (!f || !d_frame) return pt_fail(PT_EINVAL, "pt_filter_run: null %s", f ? "d_frame" : "filter");
  const size_t pixels = (size_t)f->width * f->height;
  return run_timed("pt_filter_run", f, 1, d_frame, pixels * 14, d_rgb, pixels * 3, samples, d_counts, ms_out);
}

#if PT_BUILD_EXPERIMENTS
int pt_debug_filter_tiled(pt_filter* f, int on) {
  if (!f) return pt_fail(PT_EINVAL, "pt_debug_filter_tiled: null filter");
  f->tiled = on != 0;
  return PT_OK;
}

int pt_debug_filter_step(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, int step) {
  const size_t pixels = f ? (size_t)f->width * f->height : 0;
  int rc = check_frames_args("pt_debug_filter_step", f, 1, d_frame, pixels * 14, d_rgb, pixels * 3, samples, d_counts);
  if (rc != PT_OK) return rc;
  if (step < 1 || step > 4096) return pt_fail(PT_EINVAL, "pt_debug_filter_step: step %d outside 1 .. 4096", step);
  const Params p = make_params(f, pixels * 14, d_rgb ? pixels * 3 : pixels * 14, d_rgb ? 3 : 14, samples);
  if ((rc = launch_group(f, p, 1, d_frame, d_rgb ? d_rgb : d_frame, d_counts, samples, &step, 1, nullptr)) != PT_OK) return rc;
  PT_HIP(hipDeviceSynchronize());
  return PT_OK;
}

int pt_debug_filter_state(pt_filter* f, const float* d_frame, int samples, const uint32_t* d_counts, const int* steps, int n_steps,
                          float* d_state, float* d_guide0, float* d_guide1) {
  const char* who = "pt_debug_filter_state";
  const size_t pixels = f ? (size_t)f->width * f->height : 0;
  int rc = check_frames_args(who, f, 1, d_frame, pixels * 14, nullptr, 0, samples, d_counts);
  if (rc != PT_OK) return rc;
  if (n_steps < 0 || n_steps > 8) return pt_fail(PT_EINVAL, "%s: n_steps %d outside 0 .. 8", who, n_steps);
  if (n_steps > 0 && !steps) return pt_fail(PT_EINVAL, "%s: null steps", who);
  for (int k = 0; k < n_steps; k++)
    if (steps[k] < 1 || steps[k] > 4096) return pt_fail(PT_EINVAL, "%s: steps[%d] = %d outside 1 .. 4096", who, k, steps[k]);
  if (!d_state || !d_guide0 || !d_guide1)
    return pt_fail(PT_EINVAL, "%s: null %s", who, !d_state ? "d_state" : !d_guide0 ? "d_guide0" : "d_guide1");
  const Params p = make_params(f, pixels * 14, pixels * 14, 14, samples);
  const float4* state = nullptr;
  if ((rc = launch_group(f, p, 1, d_frame, nullptr, d_counts, samples, steps, n_steps, nullptr, &state)) != PT_OK) return rc;
  const size_t n = (size_t)f->max_frames * p.pixels, bytes = pixels * sizeof(float4);
  PT_HIP(hipMemcpy(d_state, state, bytes, hipMemcpyDeviceToDevice));
  PT_HIP(hipMemcpy(d_guide0, f->d_ws + 2 * n, bytes, hipMemcpyDeviceToDevice));
  PT_HIP(hipMemcpy(d_guide1, f->d_ws + 3 * n, bytes, hipMemcpyDeviceToDevice));
  PT_HIP(hipDeviceSynchronize());
  return PT_OK;
}
#endif

}  // extern "C"
