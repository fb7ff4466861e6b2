// pt_denoise_half.h -- the half-precision instance family of the denoising network's kernels (DENOISER.md, "Half
// precision"): fp16 operands and storage, fp32 accumulation on v_mfma_f32_32x32x16_f16, fp32 epilogues.  Included by
// pt_denoise.hip inside namespace ptdn, after the fp32 kernels, which it leaves untouched.  Every fp32 -> fp16 store
// SATURATES to +-65504 (clamp in fp32, then round to nearest even): an overflow never becomes an infinity.
#ifndef PT_DENOISE_HALF_H
#define PT_DENOISE_HALF_H

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr float HALF_MAX = 65504.0f;
constexpr int HSC = 4;  // 16-wide K chunks staged per LDS buffer (64 of K between two barriers)

struct HConvArgs {
  const _Float16* in;  // NHWC [frames][in_h][in_w][cin]
  int in_h, in_w, cin;
  const _Float16* wt;  // [K / 8][npad][8]: element j of group g, column n = W[k = 8 g + j][n], k = (ky * ks + kx) * cin + c
  int npad, ks, stride;
  int out_w, M, N;
  int nchunks, chunks_per_split;
  float* partial;  // split-K: [splits][M][npad] fp32, else null
  int epi;
  const float* bias;  // [npad], fp32 as in the fp32 mode
  const float* scale;
  const float* shift;
  _Float16* out0;  // columns [0, nsplit)
  int ld0, nsplit;
  _Float16* out1;  // columns [nsplit, N)
  int ld1;
  const _Float16* res;  // EPI_ACT: residual, [M][ld0]
  const _Float16* up;   // EPI_LAT: the coarser map [up_h][up_w][32]
  int up_h, up_w, out_h;
  const _Float16* x0;   // EPI_RGB: the stored pre-processed input (albedo = channels 6-8)
  float* rgb;           // EPI_RGB: the fp32 frame (channels 0-2) or rgb buffer
  int frames, out_hw;
  size_t frame_stride;  // EPI_RGB: floats from one frame's output to the next
};

__device__ __forceinline__ int frame_of(const HConvArgs& a, int m) { return a.frames > 1 ? m / a.out_hw : 0; }

// the one rounding of a stored value: clamp to the finite fp16 range in fp32, then convert (round to nearest even)
__device__ __forceinline__ _Float16 sat_half(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -HALF_MAX, HALF_MAX); }

// upsample() of the fp32 mode on a half coarse map: the same coordinates, weights and fp32 interpolation
__device__ __forceinline__ float upsample_h(const HConvArgs& a, int f, int pix, int n) {
  const int oy = pix / a.out_w, ox = pix - oy * a.out_w;
  int h1 = 0, w1 = 0;
  float h1l = 0.0f, w1l = 0.0f;
  if (a.out_h > 1) {
    const int q = oy * (a.up_h - 1);
    h1 = q / (a.out_h - 1);
    h1l = (float)(q - h1 * (a.out_h - 1)) / (float)(a.out_h - 1);
  }
  if (a.out_w > 1) {
    const int q = ox * (a.up_w - 1);
    w1 = q / (a.out_w - 1);
    w1l = (float)(q - w1 * (a.out_w - 1)) / (float)(a.out_w - 1);
  }
  const int hp = h1 < a.up_h - 1 ? 1 : 0, wp = w1 < a.up_w - 1 ? 1 : 0;
  const float h0l = 1.0f - h1l, w0l = 1.0f - w1l;
  const _Float16* p = a.up + ((size_t)(f * a.up_h + h1) * a.up_w + w1) * 32 + n;
  const size_t dy = (size_t)hp * a.up_w * 32, dx = (size_t)wp * 32;
  return h0l * (w0l * (float)p[0] + w1l * (float)p[dx]) + h1l * (w0l * (float)p[dy] + w1l * (float)p[dy + dx]);
}

__device__ __forceinline__ void epilogue_act_h(const HConvArgs& a, int m, int n, float acc) {
  float v = __builtin_fmaf(relu(acc + a.bias[n]), a.scale[n], a.shift[n]);
  if (n < a.nsplit) {
    const size_t o = (size_t)m * a.ld0 + n;
    if (a.res) v = v + (float)a.res[o];
    a.out0[o] = sat_half(v);
  } else {
    a.out1[(size_t)m * a.ld1 + (n - a.nsplit)] = sat_half(v);
  }
}

// The epilogues of the fp32 mode, computed in fp32 from half inputs and rounded once on the store; the head writes fp32.
__device__ __forceinline__ void epilogue_h(const HConvArgs& a, int m, int n, float acc) {
  if (a.epi == EPI_ACT) {
    epilogue_act_h(a, m, n, acc);
  } else if (a.epi == EPI_LAT) {
    const float v = relu(acc + a.bias[n]);
    const int f = frame_of(a, m);
    a.out0[(size_t)m * a.ld0 + n] = sat_half(upsample_h(a, f, m - f * a.out_hw, n) + v);
  } else {
    float v = acc + a.bias[n];
    v = v * (KEPS + (float)a.x0[(size_t)m * XC + 6 + n]);
    const int f = frame_of(a, m);
    a.rgb[(size_t)f * a.frame_stride + (size_t)(m - f * a.out_hw) * a.ld0 + n] = fminf(fmaxf(v, 0.0f), 1.0f);
  }
}

// conv_kernel's implicit GEMM on v_mfma_f32_32x32x16_f16: one MFMA consumes a whole 16-wide K chunk.  Lane (r = lane & 31,
// h = lane >> 5) supplies A[row r][k = 8 h + j], j = 0..7 -- 8 consecutive channels of its pixel, ONE 16-byte load from the
// NHWC half activation -- and B[k = 8 h + j][column r], 16 contiguous bytes of the [K / 8][npad][8] weights, read from an
// LDS stage of HSC chunks ([2 HSC groups][BN columns][8]) that the 4 waves share, double-buffered.  The chunks of a slice
// are accumulated in order, one MFMA each, whatever the tile shape: an output's bits depend on the K slicing alone.
template <int TM, int TN, int WM, int WN>
__global__ void __launch_bounds__(256) hconv_kernel(HConvArgs a) {
  static_assert(WM * WN == 4, "four waves");
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int ROWS = 2 * HSC, UNITS = ROWS * BN, UPT = UNITS / 256;  // 16-byte units of a stage, per thread
  static_assert(UNITS % 256 == 0, "whole units per thread");
  __shared__ half8 Bs[2][UNITS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  const int h = lane >> 5, r = lane & 31;
  const int m0 = blockIdx.x * BM + wm * 32 * TM;
  const int nb = blockIdx.y * BN, nw = wn * 32 * TN;
  const int split = blockIdx.z;
  const int c_begin = split * a.chunks_per_split;
  const int c_end = min(a.nchunks, c_begin + a.chunks_per_split);
  const int pad = a.ks >> 1;

  int iy0[TM], ix0[TM], iyb[TM];
  bool mv[TM];
#pragma unroll
  for (int i = 0; i < TM; i++) {
    const int m = m0 + i * 32 + r;
    mv[i] = m < a.M;
    const int mm = mv[i] ? m : 0;
    const int f = frame_of(a, mm), pix = mm - f * a.out_hw;
    const int oy = pix / a.out_w, ox = pix - oy * a.out_w;
    iyb[i] = f * a.in_h;
    iy0[i] = oy * a.stride - pad;
    ix0[i] = ox * a.stride - pad;
  }
  // A fragments of the stage that starts at chunk c (zeros outside the image and past the slice's end)
#define PTDN_HLOAD_A(c, ra)                                                                                       \
  do {                                                                                                            \
    _Pragma("unroll") for (int s_ = 0; s_ < HSC; s_++) {                                                          \
      const int k0_ = ((c) + s_) * BK;                                                                            \
      const int t_ = k0_ / a.cin, ch_ = k0_ - t_ * a.cin + h * 8;                                                 \
      const int ky_ = t_ / a.ks, kx_ = t_ - ky_ * a.ks;                                                           \
      _Pragma("unroll") for (int i = 0; i < TM; i++) {                                                            \
        const int iy = iy0[i] + ky_, ix = ix0[i] + kx_;                                                           \
        half8 v_ = {0, 0, 0, 0, 0, 0, 0, 0};                                                                      \
        if ((c) + s_ < c_end && mv[i] && (unsigned)iy < (unsigned)a.in_h && (unsigned)ix < (unsigned)a.in_w)      \
          v_ = *reinterpret_cast<const half8*>(a.in + ((size_t)(iyb[i] + iy) * a.in_w + ix) * a.cin + ch_);       \
        ra[i][s_] = v_;                                                                                           \
      }                                                                                                           \
    }                                                                                                             \
  } while (0)
  // B stage: unit u = (group row, column) of the stage; rows past the slice's end are not read (nor used)
#define PTDN_HLOAD_B(c, rb)                                                                                       \
  do {                                                                                                            \
    _Pragma("unroll") for (int q_ = 0; q_ < UPT; q_++) {                                                          \
      const int u_ = tid + q_ * 256, row_ = u_ / BN, col_ = u_ - row_ * BN;                                       \
      if (2 * (c) + row_ < 2 * c_end)                                                                             \
        rb[q_] = *reinterpret_cast<const half8*>(a.wt + ((size_t)(2 * (c) + row_) * a.npad + nb + col_) * 8);     \
    }                                                                                                             \
  } while (0)
#define PTDN_HSTORE_B(buf, rb)                                                                                    \
  do {                                                                                                            \
    _Pragma("unroll") for (int q_ = 0; q_ < UPT; q_++) Bs[buf][tid + q_ * 256] = rb[q_];                          \
  } while (0)

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

  if (c_begin < c_end) {
    half8 ra[TM][HSC], rb[UPT];
#pragma unroll
    for (int q = 0; q < UPT; q++) rb[q] = half8{0, 0, 0, 0, 0, 0, 0, 0};
    PTDN_HLOAD_A(c_begin, ra);
    PTDN_HLOAD_B(c_begin, rb);
    PTDN_HSTORE_B(0, rb);
    __syncthreads();
    int buf = 0;
    for (int c = c_begin; c < c_end; c += HSC, buf ^= 1) {
      const bool more = c + HSC < c_end;
      half8 na[TM][HSC];
      if (more) {
        PTDN_HLOAD_A(c + HSC, na);
        PTDN_HLOAD_B(c + HSC, rb);
      }
      const half8* bs = Bs[buf] + h * BN + nw + r;
#pragma unroll
      for (int s = 0; s < HSC; s++) {
        if (c + s < c_end) {  // uniform over the workgroup
          half8 bv[TN];
#pragma unroll
          for (int j = 0; j < TN; j++) bv[j] = bs[2 * s * BN + j * 32];
#pragma unroll
          for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ra[i][s], bv[j], acc[i][j], 0, 0, 0);
        }
      }
      if (more) {
        PTDN_HSTORE_B(buf ^ 1, rb);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int s = 0; s < HSC; s++) ra[i][s] = na[i][s];
      }
      __syncthreads();
    }
  }
#undef PTDN_HLOAD_A
#undef PTDN_HLOAD_B
#undef PTDN_HSTORE_B

  // C/D map of the 32x32 MFMA (the same for every operand type): column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int n = nb + nw + j * 32 + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int m = m0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (m >= a.M) continue;
        if (a.partial)
          a.partial[((size_t)split * a.M + m) * a.npad + n] = acc[i][j][e];
        else if (BN > 32)  // wide tiles only serve affine layers (launch_conv checks)
          epilogue_act_h(a, m, n, acc[i][j][e]);
        else
          epilogue_h(a, m, n, acc[i][j][e]);
      }
    }
}

// splitk_reduce_kernel's half-storing twin: fp32 partials added in slice order, then the half epilogue.
__global__ void __launch_bounds__(256) hsplitk_reduce_kernel(HConvArgs a, int splits) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint32_t)a.M * (uint32_t)a.N) return;
  const int m = (int)(idx / (uint32_t)a.N), n = (int)(idx - (uint32_t)m * (uint32_t)a.N);
  float s = a.partial[(size_t)m * a.npad + n];
  for (int z = 1; z < splits; z++) s = s + a.partial[((size_t)z * a.M + m) * a.npad + n];
  epilogue_h(a, m, n, s);
}

// pre_apply_kernel's half twin: the frame receives exactly what the fp32 mode writes (channels 9-13 divided in fp32); only
// the workspace copy x0 ([frame][pixel][16] halves, two 16-byte stores) is rounded, saturating.
__global__ void __launch_bounds__(256) hpre_apply_kernel(float* __restrict__ frames, size_t frame_stride, uint32_t pixels,
                                                        const float* __restrict__ part, int nparts, _Float16* __restrict__ x0,
                                                        int inplace) {
  __shared__ float div[5];
  if (threadIdx.x < 5) {
    float m = -INFINITY;
    const float* fp = part + (size_t)blockIdx.y * nparts * 5;
    for (int b = 0; b < nparts; b++) m = fmaxf(m, fp[b * 5 + threadIdx.x]);
    div[threadIdx.x] = (float)(0.00316 + (double)m);
  }
  __syncthreads();
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= pixels) return;
  float* c = frames + blockIdx.y * frame_stride + (size_t)p * 14;
  float v[XC];
#pragma unroll
  for (int k = 0; k < 14; k++) v[k] = c[k];
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = v[k] / (KEPS + v[6 + k]);
#pragma unroll
  for (int k = 0; k < 5; k++) v[9 + k] = v[9 + k] / div[k];
  v[14] = v[15] = 0.0f;
  half8* o = reinterpret_cast<half8*>(x0 + ((size_t)blockIdx.y * pixels + p) * XC);
#pragma unroll
  for (int q = 0; q < 2; q++) {
    half8 w;
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = sat_half(v[8 * q + k]);
    o[q] = w;
  }
  if (inplace)
#pragma unroll
    for (int k = 0; k < 5; k++) c[9 + k] = v[9 + k];
}

#endif  // PT_DENOISE_HALF_H
