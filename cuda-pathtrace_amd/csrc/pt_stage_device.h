// pt_stage_device.h -- the device code that the exact post-process stages share (pt_tonemap.hip, pt_compare.hip, pt_patches.hip): the luminance
// and the integer sum over a workgroup, which is exact in any order.  EXACT code, like the kernels that use it: no contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pt_stage {

#pragma clang fp contract(off)

__device__ __forceinline__ float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // (lane 0 holds the sum)
}

// the sum over the BLOCK lanes of a workgroup, valid in thread 0; `red` holds one word per wave
template <int BLOCK>
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous use of red is over)
  if (lane == 0) red[wave] = v;
  __syncthreads();
  uint64_t s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) s += red[w];
  }
  return s;
}

}  // namespace pt_stage
