// pt_adaptive.hip -- adaptive sampling of progressive sessions: which pixels the next pass renders, and the frame afterwards.
//
// The rule, the dilation and the contract are stated in include/ptcore.h (pt_progressive_set_adaptive) and EXACTNESS.md A.20.
// Before every pass of an adaptive session, on the pass's stream and with no read-back:
//   1. classify  (one lane per tile pixel): mask bit 1 = active in the last pass and not converged at n samples;
//   2. decide    (one lane per tile pixel): mask bit 2 = active and an unconverged pixel in its window; per 256-pixel block the
//                number of such pixels (wave ballots);
//   3. scan      (one workgroup): the blocks' exclusive prefix, the list length and the maximum count;
//   4. scatter   (one lane per tile pixel): the active pixels in raster order into the list (mbcnt within a wave, the waves'
//                totals within the block, the block's prefix), their counts, and mask bit 0 = active.
// Two passes over the blocks and no look-back: nothing waits on another workgroup.  The pass itself (pixel_kernel, ADAPTIVE)
// then renders the listed pixels, and finalize forms the frame of every pixel at its own count from the record.
#include "pt_scene_lds.h"

#pragma clang fp contract(off)

namespace pt {

// the pixel's frame values at its count, exactly as pixel_kernel's epilogue forms them (frame_values): the record holds the
// state the epilogue saw, words as pixel_kernel's RESUME store
__device__ __forceinline__ void record_frame(const uint32_t* __restrict__ rec, uint32_t tile_pixels, uint32_t p, int n, float px[14]) {
  auto ld = [&](int w) { return rec[(size_t)w * tile_pixels + p]; };
  auto ldf = [&](int w) { return __uint_as_float(ld(w)); };
  TraceOutput L{mk3(ldf(PT_REC_COLOR), ldf(PT_REC_COLOR + 1), ldf(PT_REC_COLOR + 2)), mk3(ldf(PT_REC_NORMAL), ldf(PT_REC_NORMAL + 1), ldf(PT_REC_NORMAL + 2)),
                mk3(ldf(PT_REC_ALBEDO), ldf(PT_REC_ALBEDO + 1), ldf(PT_REC_ALBEDO + 2)), ldf(PT_REC_DEPTH)};
  const int n0 = (int)ld(PT_REC_N_COLOR), n1 = (int)ld(PT_REC_N_HIT);
  Welford var[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int nk = k == 0 ? n0 : n1;
    // (an opaque copy per accumulator: told that the three first-hit counts are equal, the compiler merges their variances into
    // one if/else whose else arm sits in front of the exec restore -- the shape tools/isa_exec_lint.py refuses, EXACTNESS.md A.12)
    if (k > 1) asm volatile("" : "+v"(nk));
    var[k] = Welford{nk, ldf(PT_REC_MEAN + 2 * k), ldf(PT_REC_M2 + 2 * k)};
  }
  frame_values(L, var, (float)n, px);
}

// mode: 0 = evaluate the rule, 1 = keep mask bit 0 (forced set), 2 = every pixel is active (first pass)
__global__ void __launch_bounds__(PT_ADAPTIVE_BLOCK) adaptive_classify_kernel(const uint32_t* __restrict__ rec, uint8_t* __restrict__ mask,
                                                                             uint32_t tile_pixels, int n, int mode, AdaptiveRule rule) {
  const uint32_t p = blockIdx.x * PT_ADAPTIVE_BLOCK + threadIdx.x;
  if (p >= tile_pixels) return;
  const bool act = mode == 2 ? true : (mask[p] & 1u) != 0u;
  bool unconv = act;
  if (mode == 0 && act && n >= rule.min_samples) {
    const uint32_t n0 = rec[(size_t)PT_REC_N_COLOR * tile_pixels + p], n1 = rec[(size_t)PT_REC_N_HIT * tile_pixels + p];
    bool conv = n1 == 0u;  // (a) no sample hit anything
    if (!conv && n0 == (uint32_t)n) {  // (b) every sample scored (the colour variance skips escaped paths: :157-161)
      float px[14];
      record_frame(rec, tile_pixels, p, n, px);
      const float lum = luminance(mk3(px[0], px[1], px[2]));
      const double m = (double)lum > rule.floor ? (double)lum : rule.floor;
      conv = (double)px[10] <= ((rule.tolerance * rule.tolerance) * (double)n) * (m * m);
    }
    unconv = !conv;
  }
  mask[p] = (uint8_t)((act ? 1u : 0u) | (unconv ? 2u : 0u));
}

// the number of bit-2 pixels of this workgroup's 256 (wave ballots, then the four waves' totals through LDS)
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t* s_waves, uint32_t& wave_off, uint32_t& lane_off) {
  const uint64_t b = __builtin_amdgcn_ballot_w64(flag);
  lane_off = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_waves[wave] = (uint32_t)__builtin_popcountll(b);
  __syncthreads();
  uint32_t total = 0u;
  wave_off = 0u;
#pragma unroll
  for (int w = 0; w < PT_ADAPTIVE_BLOCK / 64; w++) {
    if (w < wave) wave_off += s_waves[w];
    total += s_waves[w];
  }
  return total;
}

__global__ void __launch_bounds__(PT_ADAPTIVE_BLOCK) adaptive_decide_kernel(uint8_t* __restrict__ mask, uint32_t* __restrict__ block_sums,
                                                                           uint32_t tile_pixels, int width, int radius) {
  __shared__ uint32_t s_waves[PT_ADAPTIVE_BLOCK / 64];
  const uint32_t p = blockIdx.x * PT_ADAPTIVE_BLOCK + threadIdx.x;
  bool keep = false;
  uint8_t m = 0u;
  if (p < tile_pixels) {
    m = mask[p];
    if (m & 1u) {
      const int rows = (int)(tile_pixels / (uint32_t)width);
      const int r = (int)(p / (uint32_t)width), c = (int)(p % (uint32_t)width);
      const int r0 = r - radius < 0 ? 0 : r - radius, r1 = r + radius >= rows ? rows - 1 : r + radius;
      const int c0 = c - radius < 0 ? 0 : c - radius, c1 = c + radius >= width ? width - 1 : c + radius;
      for (int y = r0; y <= r1 && !keep; y++)
        for (int x = c0; x <= c1; x++)
          if (mask[(size_t)y * width + x] & 2u) {  // (only bit 1 is read across lanes; this kernel changes only bit 2)
            keep = true;
            break;
          }
    }
  }
  uint32_t wave_off, lane_off;
  const uint32_t total = block_count(keep, s_waves, wave_off, lane_off);
  if (p < tile_pixels && keep) mask[p] = (uint8_t)(m | 4u);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup of 1024 lanes: block_sums becomes its exclusive prefix; words[0] = list length, words[1] = the maximum count
// (n_end; 0 = leave it: a peek)
#define PT_ADAPTIVE_SCAN_THREADS 1024
__global__ void __launch_bounds__(PT_ADAPTIVE_SCAN_THREADS) adaptive_scan_kernel(uint32_t* __restrict__ block_sums, uint32_t n_blocks,
                                                                                uint32_t* __restrict__ words, int n_end) {
  __shared__ uint32_t s_waves[PT_ADAPTIVE_SCAN_THREADS / 64];
  const uint32_t per = (n_blocks + PT_ADAPTIVE_SCAN_THREADS - 1) / PT_ADAPTIVE_SCAN_THREADS;
  const uint32_t b0 = threadIdx.x * per, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
  uint32_t mine = 0u;
  for (uint32_t b = b0; b < b1; b++) mine += block_sums[b];
  // inclusive scan of `mine` within the wave, then over the waves
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (lane == 63) s_waves[wave] = incl;
  __syncthreads();
  uint32_t off = 0u, total = 0u;
  for (int w = 0; w < PT_ADAPTIVE_SCAN_THREADS / 64; w++) {
    if (w < wave) off += s_waves[w];
    total += s_waves[w];
  }
  uint32_t run = off + incl - mine;
  for (uint32_t b = b0; b < b1; b++) {
    const uint32_t v = block_sums[b];
    block_sums[b] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    words[0] = total;
    if (total > 0u && n_end > 0) words[1] = (uint32_t)n_end;
  }
}

__global__ void __launch_bounds__(PT_ADAPTIVE_BLOCK) adaptive_scatter_kernel(uint8_t* __restrict__ mask, const uint32_t* __restrict__ block_sums,
                                                                            uint32_t* __restrict__ list, uint32_t* __restrict__ counts,
                                                                            uint32_t tile_pixels, int n_end) {
  __shared__ uint32_t s_waves[PT_ADAPTIVE_BLOCK / 64];
  const uint32_t p = blockIdx.x * PT_ADAPTIVE_BLOCK + threadIdx.x;
  const bool keep = p < tile_pixels && (mask[p] & 4u) != 0u;
  uint32_t wave_off, lane_off;
  (void)block_count(keep, s_waves, wave_off, lane_off);
  if (p < tile_pixels) {
    if (keep) {
      list[block_sums[blockIdx.x] + wave_off + lane_off] = p;
      counts[p] = (uint32_t)n_end;
    }
    mask[p] = keep ? 1u : 0u;
  }
}

// every tile pixel's 14 channels at its own count
__global__ void __launch_bounds__(PT_ADAPTIVE_BLOCK) adaptive_finalize_kernel(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ counts,
                                                                             float* __restrict__ out, uint32_t tile_pixels, uint32_t planar) {
  const uint32_t p = blockIdx.x * PT_ADAPTIVE_BLOCK + threadIdx.x;
  if (p >= tile_pixels) return;
  float px[14];
  record_frame(rec, tile_pixels, p, (int)counts[p], px);
  if (planar) {
#pragma unroll
    for (int c = 0; c < 14; c++) out[(size_t)c * tile_pixels + p] = px[c];
  } else {
    float* o = out + (size_t)p * 14;
#pragma unroll
    for (int c = 0; c < 14; c++) o[c] = px[c];
  }
}

}  // namespace pt

hipError_t pt_launch_adaptive_select(const AdaptiveState& s, const AdaptiveRule& rule, const uint32_t* rec, uint32_t tile_pixels,
                                     int width, int n, int n_end, int mode, bool peek, hipStream_t stream) {
  if (!tile_pixels) return hipSuccess;
  if (!s.counts || !s.list || !s.mask || !s.block_sums || !s.words || !rec || width < 1 || tile_pixels % (uint32_t)width != 0u ||
      mode < 0 || mode > 2 || rule.radius < 0 || n < 0 || n_end <= n)
    return hipErrorInvalidValue;
  const uint32_t n_blocks = (tile_pixels + PT_ADAPTIVE_BLOCK - 1) / PT_ADAPTIVE_BLOCK;
  hipLaunchKernelGGL(pt::adaptive_classify_kernel, dim3(n_blocks), dim3(PT_ADAPTIVE_BLOCK), 0, stream, rec, s.mask, tile_pixels, n, mode, rule);
  hipLaunchKernelGGL(pt::adaptive_decide_kernel, dim3(n_blocks), dim3(PT_ADAPTIVE_BLOCK), 0, stream, s.mask, s.block_sums, tile_pixels, width,
                     rule.radius);
  hipLaunchKernelGGL(pt::adaptive_scan_kernel, dim3(1), dim3(PT_ADAPTIVE_SCAN_THREADS), 0, stream, s.block_sums, n_blocks, s.words,
                     peek ? 0 : n_end);
  if (peek) return hipGetLastError();
  hipLaunchKernelGGL(pt::adaptive_scatter_kernel, dim3(n_blocks), dim3(PT_ADAPTIVE_BLOCK), 0, stream, s.mask, s.block_sums, s.list, s.counts,
                     tile_pixels, n_end);
  return hipGetLastError();
}

hipError_t pt_launch_adaptive_finalize(const uint32_t* rec, const uint32_t* counts, float* out, uint32_t tile_pixels, bool planar,
                                       hipStream_t stream) {
  if (!tile_pixels) return hipSuccess;
  if (!rec || !counts || !out) return hipErrorInvalidValue;
  const uint32_t n_blocks = (tile_pixels + PT_ADAPTIVE_BLOCK - 1) / PT_ADAPTIVE_BLOCK;
  hipLaunchKernelGGL(pt::adaptive_finalize_kernel, dim3(n_blocks), dim3(PT_ADAPTIVE_BLOCK), 0, stream, rec, counts, out, tile_pixels,
                     planar ? 1u : 0u);
  return hipGetLastError();
}
