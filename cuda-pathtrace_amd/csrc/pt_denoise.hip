// pt_denoise.hip -- the reference's denoising network (DenoiseCNN, denoise_cnn/model.py, run by train.py:test() from the
// interactive loop, src/main.cu:92-122,146-152) as fp32 MFMA inference behind pt_denoiser_* (include/ptcore.h), and, opt-in
// (PT_DENOISE_F16), the same network on fp16 operands and storage with fp32 accumulation.  Design and numbers: DENOISER.md.
// ONE kernel family, templated on T, the element type of a stored activation (float / _Float16): the two pre-processing
// kernels (channel maxima, then the divisions and the channel-padded NHWC copy), the implicit-GEMM convolution (compile-time
// tile shape, run-time epilogue kind) and the deterministic split-K reduction that applies the same epilogue.  Everything
// outside an MFMA is computed in fp32 in both modes: T decides only how a stored value is read (widened by a cast) and
// written (to_stored: the half mode's one rounding) and which of conv_kernel's two main loops runs (32x32x2 f32 MFMA or
// 32x32x16 f16 MFMA) between the set-up and the C/D store they share.  Host side: the PTDN weight loader, the
// layer table and the workspace, fixed at create time for the denoiser's width and height and grown by
// pt_denoiser_reserve_frames for batches: a batch of n frames runs through the same launches as one frame, its rows
// m = (frame, pixel) (DENOISER.md, "Batches").
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "pt_stage.h"
#if PT_BUILD_EXPERIMENTS
#include "../../include/ptcore_lab.h"
#endif

#pragma clang fp contract(off)

namespace ptdn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

enum { EPI_ACT = 0, EPI_LAT = 1, EPI_RGB = 2 };
constexpr int BK = 16;              // K per staged chunk (every stored Cin is a multiple of 16: one chunk never straddles a tap)
constexpr int XC = 16;              // channels of the padded input copy (14 + 2 zeros)
constexpr int PRE_BLOCKS = 256;     // partial maxima of the pre-processing reduction
constexpr float KEPS = 0.00316f;    // train.py:48-55, model.py forward
constexpr float HALF_MAX = 65504.0f;
constexpr int HSC = 4;  // half GEMM: 16-wide K chunks staged per LDS buffer (64 of K between two barriers)

// Rows m = f * out_h * out_w + pixel over the `frames` frames of a group; every activation is [frames][h][w][c], contiguous.
// T = the element of a stored activation and of the convolution weights; split-K partials, bias / scale / shift and the
// head's output are fp32 in both modes.
template <class T>
struct ConvArgs {
  const T* in;  // NHWC [frames][in_h][in_w][cin]
  int in_h, in_w, cin;
  const T* wt;  // float: [K][npad], row k = (ky * ks + kx) * cin + c; _Float16: [K / 8][npad][8], element j of group g,
                // column n = W[k = 8 g + j][n]
  int npad, ks, stride;
  int out_w, M, N;
  int nchunks, chunks_per_split;
  float* partial;  // split-K: [splits][M][npad], else null
  int epi;
  const float* bias;  // [npad]
  const float* scale; // [npad] folded batch-norm (1 / 0 where there is none)
  const float* shift;
  T* out0;            // columns [0, nsplit): out0[m * ld0 + n]
  int ld0, nsplit;
  T* out1;            // columns [nsplit, N): out1[m * ld1 + n - nsplit]
  int ld1;
  const T* res;       // EPI_ACT: residual added after the affine, [M][ld0]
  const T* up;        // EPI_LAT: the coarser map [up_h][up_w][32], bilinearly upsampled (align_corners) and added
  int up_h, up_w, out_h;
  const T* x0;        // EPI_RGB: the pre-processed input (albedo = channels 6-8)
  float* rgb;         // EPI_RGB: the fp32 frame (channels 0-2) or rgb buffer; see head_out
  int frames, out_hw; // frames of the group (M = frames * out_hw)
  size_t frame_stride; // EPI_RGB: floats from one frame's output to the next (head_out + f * frame_stride + pixel * ld0)
};

// Where the head writes.  The fp32 head keeps writing through out0 (conv_args points it at the frame): loading `rgb`
// instead re-allocates the scalar registers of every fp32 kernel that holds the head epilogue.
__device__ __forceinline__ float* head_out(const ConvArgs<float>& a) { return a.out0; }
__device__ __forceinline__ float* head_out(const ConvArgs<_Float16>& a) { return a.rgb; }

// The one rounding of a stored value.  float: none.  _Float16: clamp to the finite fp16 range in fp32, then convert (round
// to nearest even), so an overflow never becomes an infinity.  Stored values are read back with a plain (float) cast.
__device__ __forceinline__ _Float16 sat_half(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -HALF_MAX, HALF_MAX); }
template <class T>
__device__ __forceinline__ T to_stored(float v) {
  if constexpr (std::is_same<T, float>::value)
    return v;
  else
    return sat_half(v);
}

// The frame of row m and the row's pixel inside it (one frame: no division).
template <class T>
__device__ __forceinline__ int frame_of(const ConvArgs<T>& a, int m) {
  return a.frames > 1 ? m / a.out_hw : 0;
}

// ReLU that returns +0 for every non-positive input (torch: x <= 0 -> 0)
__device__ __forceinline__ float relu(float v) { return v > 0.0f ? v : 0.0f; }

// F.upsample(mode='bilinear') of torch 0.2/0.3: align-corners semantics, source coordinate oy (in - 1) / (out - 1).  The
// coordinate is formed EXACTLY (integer quotient and remainder; weight = remainder / (out - 1), one rounding) rather than as
// torch's float32 scale * index, whose rounding moves a sample by up to an ulp of the coordinate (DENOISER.md); the
// interpolation itself is THNN's: h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11).
template <class T>
__device__ __forceinline__ float upsample(const ConvArgs<T>& a, int f, int pix, int n) {
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
  const T* p = a.up + ((size_t)(f * a.up_h + h1) * a.up_w + w1) * 32 + n;
  const size_t dy = (size_t)hp * a.up_w * 32, dx = (size_t)wp * 32;
  return h0l * (w0l * (float)p[0] + w1l * (float)p[dx]) + h1l * (w0l * (float)p[dy] + w1l * (float)p[dy + dx]);
}

// conv, ReLU, folded BN (ResBlock: model.py:20-30), + residual (conv2)
template <class T>
__device__ __forceinline__ void epilogue_act(const ConvArgs<T>& a, int m, int n, float acc) {
  float v = __builtin_fmaf(relu(acc + a.bias[n]), a.scale[n], a.shift[n]);
  if (n < a.nsplit) {
    const size_t o = (size_t)m * a.ld0 + n;
    if (a.res) v = v + (float)a.res[o];
    a.out0[o] = to_stored<T>(v);
  } else {
    a.out1[(size_t)m * a.ld1 + (n - a.nsplit)] = to_stored<T>(v);
  }
}

// The fused epilogue of every layer (m < M, n < N), computed in fp32 and rounded once on the store; the head writes fp32.
template <class T>
__device__ __forceinline__ void epilogue(const ConvArgs<T>& a, int m, int n, float acc) {
  if (a.epi == EPI_ACT) {
    epilogue_act(a, m, n, acc);
  } else if (a.epi == EPI_LAT) {  // upsample(rep) + ReLU(lat_k(raw_k)), model.py:72-74
    const float v = relu(acc + a.bias[n]);
    const int f = frame_of(a, m);
    a.out0[(size_t)m * a.ld0 + n] = to_stored<T>(upsample(a, f, m - f * a.out_hw, n) + v);
  } else {  // rgb head: clamp(rgb_conv(rep) * (0.00316 + albedo), 0, 1), model.py:101-103
    float v = acc + a.bias[n];
    v = v * (KEPS + (float)a.x0[(size_t)m * XC + 6 + n]);
    const int f = frame_of(a, m);
    head_out(a)[(size_t)f * a.frame_stride + (size_t)(m - f * a.out_hw) * a.ld0 + n] = fminf(fmaxf(v, 0.0f), 1.0f);
  }
}

// Implicit-GEMM convolution: rows = output pixels, columns = output channels, K = taps x Cin.  4 waves; wave (wm, wn) owns
// TM x TN tiles of 32 x 32.  blockIdx.z = split-K slice (partials to a.partial, summed in order by splitk_reduce_kernel:
// deterministic, no atomics).  Rows run over the group's frames: a window is zero-padded at its own frame's borders (iy is
// checked against in_h before the frame's first input row iyb is added).  The set-up, the accumulators and the C/D store
// are the same for both element types; each has its OWN main loop, because their staging differs for measured reasons
// (DENOISER.md, "Half precision"):
//  * float, v_mfma_f32_32x32x2_f32: inside a 16-wide K chunk, MFMA step kk takes k = kk from lane half 0 and k = 8 + kk from
//    lane half 1, so a lane's A operands for the whole chunk are 8 CONSECUTIVE channels of its pixel -- two float4 loads
//    straight from the NHWC activation, no LDS (no other wave reads those rows).  The B chunk (weights) is shared by the 4
//    waves and double-buffered in LDS.
//  * _Float16, v_mfma_f32_32x32x16_f16: one MFMA consumes a whole 16-wide K chunk.  Lane (r = lane & 31, h = lane >> 5)
//    supplies A[row r][k = 8 h + j], j = 0..7 -- 8 consecutive channels of its pixel, ONE 16-byte load from the NHWC half
//    activation -- and B[k = 8 h + j][column r], 16 contiguous bytes of the [K / 8][npad][8] weights, read from an LDS stage
//    of HSC chunks ([2 HSC groups][BN columns][8]) that the 4 waves share, double-buffered.  The chunks of a slice are
//    accumulated in order, one MFMA each, whatever the tile shape: an output's bits depend on the K slicing alone.
template <class T, int TM, int TN, int WM, int WN>
__global__ void __launch_bounds__(256) conv_kernel(ConvArgs<T> a) {
  static_assert(WM * WN == 4, "four waves");
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
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

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

  if constexpr (std::is_same<T, float>::value) {
    constexpr int LDB = BN + 4;
    constexpr int BF4 = BK * BN / 4, BPT = (BF4 + 255) / 256;
    __shared__ float4 Bs4[2][BK * LDB / 4];
    // A chunk c of this lane: 8 consecutive channels of its pixel per 32-row tile (zeros outside the image = padding)
#define PTDN_LOAD_A(c, ra)                                                                                        \
  do {                                                                                                            \
    const int k0_ = (c) * BK;                                                                                     \
    const int t_ = k0_ / a.cin, ch_ = k0_ - t_ * a.cin + h * 8;                                                   \
    const int ky_ = t_ / a.ks, kx_ = t_ - ky_ * a.ks;                                                             \
    _Pragma("unroll") for (int i = 0; i < TM; i++) {                                                              \
      const int iy = iy0[i] + ky_, ix = ix0[i] + kx_;                                                             \
      float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;                                                   \
      if (mv[i] && (unsigned)iy < (unsigned)a.in_h && (unsigned)ix < (unsigned)a.in_w) {                          \
        const float4* p_ = reinterpret_cast<const float4*>(a.in + ((size_t)(iyb[i] + iy) * a.in_w + ix) * a.cin + ch_); \
        v0 = p_[0];                                                                                               \
        v1 = p_[1];                                                                                               \
      }                                                                                                           \
      ra[i][0] = v0.x, ra[i][1] = v0.y, ra[i][2] = v0.z, ra[i][3] = v0.w;                                         \
      ra[i][4] = v1.x, ra[i][5] = v1.y, ra[i][6] = v1.z, ra[i][7] = v1.w;                                         \
    }                                                                                                             \
  } while (0)
    // B chunk c (BK x BN weights of this block's columns): float4 number tid (and tid + 256) of the chunk per thread
    static_assert(BPT <= 2, "at most two float4 of B per thread");
#define PTDN_B_ADDR(c, f) (a.wt + (size_t)((c) * BK + (f) / (BN / 4)) * a.npad + nb + ((f) % (BN / 4)) * 4)
#define PTDN_LOAD_B(c, rb0, rb1)                                                                                  \
  do {                                                                                                            \
    if (tid < BF4) rb0 = *reinterpret_cast<const float4*>(PTDN_B_ADDR(c, tid));                                   \
    if (BPT > 1 && tid + 256 < BF4) rb1 = *reinterpret_cast<const float4*>(PTDN_B_ADDR(c, tid + 256));            \
  } while (0)
#define PTDN_STORE_B(buf, rb0, rb1)                                                                               \
  do {                                                                                                            \
    if (tid < BF4) Bs4[buf][(tid / (BN / 4)) * (LDB / 4) + tid % (BN / 4)] = rb0;                                 \
    if (BPT > 1 && tid + 256 < BF4) Bs4[buf][((tid + 256) / (BN / 4)) * (LDB / 4) + (tid + 256) % (BN / 4)] = rb1; \
  } while (0)
    if (c_begin < c_end) {
      float ra[TM][8];
      float4 rb0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb1 = rb0;
      PTDN_LOAD_A(c_begin, ra);
      PTDN_LOAD_B(c_begin, rb0, rb1);
      PTDN_STORE_B(0, rb0, rb1);
      __syncthreads();
      for (int c = c_begin; c < c_end; c++) {
        const int buf = (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
        float na[TM][8];
        if (more) {
          PTDN_LOAD_A(c + 1, na);
          PTDN_LOAD_B(c + 1, rb0, rb1);
        }
        const float* bs = reinterpret_cast<const float*>(Bs4[buf]) + h * 8 * LDB + nw + r;
#pragma unroll
        for (int kk = 0; kk < 8; kk++) {
          float bv[TN];
#pragma unroll
          for (int j = 0; j < TN; j++) bv[j] = bs[kk * LDB + j * 32];
#pragma unroll
          for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[i][kk], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
          PTDN_STORE_B(buf ^ 1, rb0, rb1);
#pragma unroll
          for (int i = 0; i < TM; i++)
#pragma unroll
            for (int e = 0; e < 8; e++) ra[i][e] = na[i][e];
        }
        __syncthreads();
      }
    }
#undef PTDN_LOAD_A
#undef PTDN_LOAD_B
#undef PTDN_STORE_B
#undef PTDN_B_ADDR
  } else {
    constexpr int ROWS = 2 * HSC, UNITS = ROWS * BN, UPT = UNITS / 256;  // 16-byte units of a stage, per thread
    static_assert(UNITS % 256 == 0, "whole units per thread");
    __shared__ half8 Bs[2][UNITS];
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
  }

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
        else if (BN > 32)  // wide tiles only serve affine layers (N > 32; launch_conv checks)
          epilogue_act(a, m, n, acc[i][j][e]);
        else
          epilogue(a, m, n, acc[i][j][e]);
      }
    }
}

// Split-K: the slices' fp32 partial sums added in slice order (bit-identical from run to run), then the layer's epilogue.
template <class T>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(ConvArgs<T> a, int splits) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint32_t)a.M * (uint32_t)a.N) return;
  const int m = (int)(idx / (uint32_t)a.N), n = (int)(idx - (uint32_t)m * (uint32_t)a.N);
  float s = a.partial[(size_t)m * a.npad + n];
  for (int z = 1; z < splits; z++) s = s + a.partial[((size_t)z * a.M + m) * a.npad + n];
  epilogue(a, m, n, s);
}

// Pre-processing 1/2 (train.py:50-54): per-block maxima of channels 9-13 (a max is exact in any order).  blockIdx.y = frame
// of the group (frames frame_stride floats apart), part[frame][block][5]: every frame gets its own maxima.
__global__ void __launch_bounds__(256) pre_max_kernel(const float* __restrict__ frames, size_t frame_stride, uint32_t pixels,
                                                     float* __restrict__ part) {
  const float* frame = frames + blockIdx.y * frame_stride;
  float mx[5];
#pragma unroll
  for (int k = 0; k < 5; k++) mx[k] = -INFINITY;
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < pixels; p += gridDim.x * 256u)
#pragma unroll
    for (int k = 0; k < 5; k++) mx[k] = fmaxf(mx[k], frame[(size_t)p * 14 + 9 + k]);
#pragma unroll
  for (int k = 0; k < 5; k++)
    for (int s = 1; s < 64; s <<= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], s));
  __shared__ float wmx[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 5; k++) wmx[wave][k] = mx[k];
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 5 + k] = fmaxf(fmaxf(wmx[0][k], wmx[1][k]), fmaxf(wmx[2][k], wmx[3][k]));
  }
}

// Pre-processing 2/2 (train.py:48-55): colour / (0.00316 + albedo); channel k of 9-13 / (float)(0.00316 + (double)max_k) --
// the divisor of torch 0.2/0.3, whose torch.max(t) returned a Python float.  Writes the 16-channel NHWC copy the network
// reads (channels 14, 15 = 0) and, in place, the normalised channels 9-13 back into the frame (channels 3-8 are unchanged,
// 0-2 are overwritten by the rgb head).  blockIdx.y = frame of the group, divided by its own maxima; x0 is [frame][pixel][16].
// The frame receives the same fp32 values in both modes; only the workspace copy x0 is stored as T (16-byte stores).
template <class T>
__global__ void __launch_bounds__(256) pre_apply_kernel(float* __restrict__ frames, size_t frame_stride, uint32_t pixels,
                                                       const float* __restrict__ part, int nparts, T* __restrict__ x0, int inplace) {
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
  constexpr int VE = 16 / sizeof(T);  // elements of a 16-byte store
  typedef T vec __attribute__((ext_vector_type(VE)));
  vec* o = reinterpret_cast<vec*>(x0 + ((size_t)blockIdx.y * pixels + p) * XC);
#pragma unroll
  for (int q = 0; q < XC / VE; q++) {
    vec w;
#pragma unroll
    for (int k = 0; k < VE; k++) w[k] = to_stored<T>(v[VE * q + k]);
    o[q] = w;
  }
  if (inplace)
#pragma unroll
    for (int k = 0; k < 5; k++) c[9 + k] = v[9 + k];
}

// ---- host side -------------------------------------------------------------------------------------------------------------
const int kChannels[7] = {14, 32, 64, 128, 256, 512, 1024};

struct Tensor {
  std::vector<uint32_t> shape;
  const unsigned char* data;  // little-endian float32, unaligned
  size_t count;
};

// name -> shape of every tensor of the network (denoise_weights.expected_shapes() restates it)
static std::map<std::string, std::vector<uint32_t>> expected_shapes() {
  std::map<std::string, std::vector<uint32_t>> out;
  char name[64];
  for (int b = 1; b <= 6; b++) {
    const uint32_t cin = kChannels[b - 1], cout = kChannels[b];
    const char* convs[3] = {"res_conv", "conv1", "conv2"};
    for (int c = 0; c < 3; c++) {
      snprintf(name, sizeof(name), "block%d.%s.weight", b, convs[c]);
      out[name] = {cout, c == 2 ? cout : cin, 3, 3};
      snprintf(name, sizeof(name), "block%d.%s.bias", b, convs[c]);
      out[name] = {cout};
    }
    const char* bns[3] = {"res_bn", "bn1", "bn2"};
    const char* ps[4] = {"weight", "bias", "running_mean", "running_var"};
    for (int n = 0; n < 3; n++)
      for (int p = 0; p < 4; p++) {
        snprintf(name, sizeof(name), "block%d.%s.%s", b, bns[n], ps[p]);
        out[name] = {cout};
      }
  }
  for (int k = 0; k <= 6; k++) {
    snprintf(name, sizeof(name), "lat_%d.weight", k);
    out[name] = {32, (uint32_t)kChannels[k], 1, 1};
    snprintf(name, sizeof(name), "lat_%d.bias", k);
    out[name] = {32};
    if (k < 6) {
      snprintf(name, sizeof(name), "backwards_%d%d.weight", k + 1, k);
      out[name] = {32, 32, 3, 3};
      snprintf(name, sizeof(name), "backwards_%d%d.bias", k + 1, k);
      out[name] = {32};
    }
  }
  out["rgb_conv.weight"] = {3, 32, 3, 3};
  out["rgb_conv.bias"] = {3};
  return out;
}

static std::string shape_str(const std::vector<uint32_t>& s) {
  std::string o = "(";
  for (size_t i = 0; i < s.size(); i++) o += (i ? ", " : "") + std::to_string(s[i]);
  return o + (s.size() == 1 ? ",)" : ")");
}

// Parses and checks a PTDN image (layout: include/ptcore.h).  Every expected tensor present once with its shape, nothing
// else, no trailing bytes; the message names the offending key.
static int parse_weights(const void* blob, size_t bytes, std::map<std::string, Tensor>* out, const char* who) {
  if (!blob) return pt_fail(PT_EINVAL, "%s: null weight blob", who);
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  size_t off = 0;
  auto u32 = [&](uint32_t* v) {
    if (bytes - off < 4) return false;
    memcpy(v, p + off, 4);  // little-endian hosts only (x86-64)
    off += 4;
    return true;
  };
  uint32_t version = 0, n = 0;
  if (bytes < 12 || memcmp(p, "PTDN", 4) != 0) return pt_fail(PT_EINVAL, "%s: not a PTDN weight file (bad magic)", who);
  off = 4;
  u32(&version);
  u32(&n);
  if (version != 1) return pt_fail(PT_EINVAL, "%s: PTDN version %u is not supported (1 is)", who, version);
  const auto want = expected_shapes();
  std::map<std::string, Tensor> got;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t len = 0, nd = 0;
    if (!u32(&len) || bytes - off < len) return pt_fail(PT_EINVAL, "%s: truncated file (in the name of tensor %u)", who, i);
    std::string name(reinterpret_cast<const char*>(p + off), len);
    off += len;
    if (!u32(&nd) || nd > 8) return pt_fail(PT_EINVAL, "%s: truncated or corrupt header of tensor '%s'", who, name.c_str());
    Tensor t;
    t.count = 1;
    for (uint32_t d = 0; d < nd; d++) {
      uint32_t v = 0;
      if (!u32(&v)) return pt_fail(PT_EINVAL, "%s: truncated shape of tensor '%s'", who, name.c_str());
      t.shape.push_back(v);
      t.count *= v;
    }
    if (t.count > (bytes - off) / 4) return pt_fail(PT_EINVAL, "%s: truncated data of tensor '%s'", who, name.c_str());
    t.data = p + off;
    off += t.count * 4;
    auto w = want.find(name);
    if (w == want.end()) return pt_fail(PT_EINVAL, "%s: unexpected tensor '%s'", who, name.c_str());
    if (got.count(name)) return pt_fail(PT_EINVAL, "%s: tensor '%s' appears twice", who, name.c_str());
    if (t.shape != w->second)
      return pt_fail(PT_EINVAL, "%s: tensor '%s' has shape %s, expected %s", who, name.c_str(), shape_str(t.shape).c_str(),
                     shape_str(w->second).c_str());
    got[name] = t;
  }
  if (off != bytes) return pt_fail(PT_EINVAL, "%s: %zu trailing bytes after the last tensor", who, bytes - off);
  for (const auto& w : want)
    if (!got.count(w.first)) return pt_fail(PT_EINVAL, "%s: missing tensor '%s'", who, w.first.c_str());
  if (out) *out = got;
  return PT_OK;
}

static float ld_f32(const Tensor& t, size_t i) {
  float v;
  memcpy(&v, t.data + 4 * i, 4);
  return v;
}

struct Act {
  std::string name;
  int h, w, c;
  size_t off;  // floats into the workspace: [max_frames][h][w][c], frame 0 first
};

struct Conv {
  std::string name;
  int in, out0, out1, res, up;  // activation ids (-1: none); out0 = -1: the frame / rgb buffer (rgb head)
  int cin, ks, stride, N, nsplit, epi;
  int in_h, in_w, out_h, out_w, M, K;
  int cfg, npad, splits, chunks_per_split, nchunks;
  size_t w_off;  // floats into the host weight image: wt [K][npad], bias, scale, shift [npad] each
  size_t p_off;  // floats into d_w: bias, scale, shift (fp32 mode: w_off + K * npad, behind wt; half mode: packed)
  size_t h_off;  // half mode: halves into d_wh, wt [K / 8][npad][8]
};

struct TileCfg {
  int bm, bn;
};
// conv_kernel<T, TM, TN, WM, WN> instances: 256x32, 128x64, 128x128 for large layers, 128x32 and 64x64 for small ones (+ split-K)
static const TileCfg kCfg[5] = {{256, 32}, {128, 64}, {128, 128}, {128, 32}, {64, 64}};

// The plan table of each precision: the tile shape of a layer (the wide tile of its column class when the layer fills at
// least `wide_tiles` of them, else the small one) and its K slicing (split until `target_wgs` workgroups are in flight, at
// least `min_chunks` 16-wide chunks per slice).  Half: an fp16 MFMA retires a chunk in 1/16 of the time and the kernel
// stages 4 chunks between two barriers, so a slice is at least 16 chunks (256 of K, 4 stages) to be worth its fp32
// partials and its reduction (DENOISER.md, "Half precision").
struct PlanRule {
  int wide_tiles[3];  // N <= 32, N <= 64, N > 64
  int target_wgs, min_chunks;
};
static const PlanRule kPlan[2] = {{{256, 128, 256}, 512, 8}, {{256, 128, 256}, 512, 16}};

}  // namespace ptdn

using namespace ptdn;

struct pt_denoiser {
  int width, height, device;
  std::vector<Act> acts;
  std::vector<Conv> convs;
  int precision = PT_DENOISE_F32;
  size_t esz = sizeof(float);                 // bytes of a stored activation element
  float* d_w = nullptr;                       // fp32: weights + bias/scale/shift; half: bias/scale/shift only
  _Float16* d_wh = nullptr;                   // half: the convolution weights
  char* d_ws = nullptr;                       // activations, ws_elems elements of esz bytes
  float* d_partial = nullptr;
  float* d_premax = nullptr;
  size_t ws_elems = 0, w_floats = 0, partial_floats = 0, p_floats = 0, wh_halves = 0;
  int pre_blocks = 0;
  int max_frames = 1;                         // frames per group (pt_denoiser_reserve_frames)
  std::map<int, std::vector<Conv>> plans;     // batch_plan of each group size used so far
  int last_groups = 0, last_launches = 0;     // of the last enqueue (lab getter)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static int64_t conv_tiles(const Conv& c, int cfg) {
  const int bn = kCfg[cfg].bn;
  return (int64_t)((c.M + kCfg[cfg].bm - 1) / kCfg[cfg].bm) * ((c.N + bn - 1) / bn);
}

static int pick_cfg(const Conv& c, const PlanRule& p) {
  if (c.N <= 32) return conv_tiles(c, 0) >= p.wide_tiles[0] ? 0 : 3;
  if (c.N <= 64) return conv_tiles(c, 1) >= p.wide_tiles[1] ? 1 : 4;
  return conv_tiles(c, 2) >= p.wide_tiles[2] ? 2 : 4;
}

static void choose_tiles(Conv& c, const PlanRule& p) {
  c.cfg = pick_cfg(c, p);
  c.npad = (c.N + kCfg[c.cfg].bn - 1) / kCfg[c.cfg].bn * kCfg[c.cfg].bn;
  c.nchunks = c.K / BK;
  // split K until about two workgroups per CU are in flight, keeping at least PlanRule::min_chunks chunks per slice (8 =
  // 128 of K in fp32, 16 = 256 of K in half)
  const int64_t t = conv_tiles(c, c.cfg);
  int splits = 1;
  if (t < p.target_wgs / 2) {
    splits = (int)((p.target_wgs + t - 1) / t);
    const int most = c.nchunks / p.min_chunks > 0 ? c.nchunks / p.min_chunks : 1;
    if (splits > most) splits = most;
  }
  c.chunks_per_split = (c.nchunks + splits - 1) / splits;
  c.splits = (c.nchunks + c.chunks_per_split - 1) / c.chunks_per_split;
}

// Layer table for a width x height frame (H = rows): activations and convolutions in execution order.
static void build_layers(pt_denoiser* d) {
  int sh[7], sw[7];
  sh[0] = d->height;
  sw[0] = d->width;
  for (int b = 1; b <= 6; b++) sh[b] = (sh[b - 1] + 1) / 2, sw[b] = (sw[b - 1] + 1) / 2;
  auto act = [&](const std::string& n, int h, int w, int c) {
    d->acts.push_back({n, h, w, c, 0});
    return (int)d->acts.size() - 1;
  };
  int raw[7];
  raw[0] = act("input", sh[0], sw[0], XC);
  auto conv = [&](const std::string& n, int in, int ks, int stride, int N, int epi, int out0, int nsplit, int out1, int res, int up) {
    Conv c{};
    c.name = n;
    c.in = in, c.out0 = out0, c.out1 = out1, c.res = res, c.up = up;
    const Act& a = d->acts[in];
    c.cin = a.c, c.ks = ks, c.stride = stride, c.N = N, c.nsplit = nsplit, c.epi = epi;
    c.in_h = a.h, c.in_w = a.w;
    c.out_h = (a.h - 1) / stride + 1, c.out_w = (a.w - 1) / stride + 1;
    c.M = c.out_h * c.out_w;
    c.K = ks * ks * c.cin;
    choose_tiles(c, kPlan[d->precision]);
    d->convs.push_back(c);
  };
  char n[64];
  for (int b = 1; b <= 6; b++) {
    const int C = kChannels[b];
    snprintf(n, sizeof(n), "block%d.t1", b);
    const int t1 = act(n, sh[b], sw[b], C);
    snprintf(n, sizeof(n), "block%d.res", b);
    const int rs = act(n, sh[b], sw[b], C);
    snprintf(n, sizeof(n), "block%d.out", b);
    raw[b] = act(n, sh[b], sw[b], C);
    snprintf(n, sizeof(n), "block%d.conv1+res_conv", b);
    conv(n, raw[b - 1], 3, 2, 2 * C, EPI_ACT, t1, C, rs, -1, -1);
    snprintf(n, sizeof(n), "block%d.conv2", b);
    conv(n, t1, 3, 1, C, EPI_ACT, raw[b], C, -1, rs, -1);
  }
  int rep = act("lat6", sh[6], sw[6], 32);
  conv("lat_6", raw[6], 1, 1, 32, EPI_ACT, rep, 32, -1, -1, -1);
  for (int k = 5; k >= 0; k--) {
    snprintf(n, sizeof(n), "back%d%d", k + 1, k);
    const int bk = act(n, (d->acts[rep].h + 1) / 2, (d->acts[rep].w + 1) / 2, 32);
    snprintf(n, sizeof(n), "backwards_%d%d", k + 1, k);
    conv(n, rep, 3, 2, 32, EPI_ACT, bk, 32, -1, -1, -1);
    snprintf(n, sizeof(n), "rep%d", k);
    const int nr = act(n, sh[k], sw[k], 32);
    snprintf(n, sizeof(n), "lat_%d", k);
    conv(n, raw[k], 1, 1, 32, EPI_LAT, nr, 32, -1, -1, bk);
    rep = nr;
  }
  conv("rgb_conv", rep, 3, 1, 3, EPI_RGB, -1, 3, -1, -1, -1);
  size_t woff = 0, poff = 0, hoff = 0;
  for (Conv& c : d->convs) {
    c.w_off = woff;
    woff += ((size_t)c.K * c.npad + 3 * (size_t)c.npad + 63) / 64 * 64;
    c.h_off = hoff;
    hoff += ((size_t)c.K * c.npad + 127) / 128 * 128;
    c.p_off = d->precision == PT_DENOISE_F16 ? poff : c.w_off + (size_t)c.K * c.npad;
    poff += (3 * (size_t)c.npad + 63) / 64 * 64;
  }
  d->w_floats = woff, d->p_floats = poff, d->wh_halves = hoff;
}

// The conv table of a group of n frames, from the single-frame table: M = n rows per output pixel, the tile shape re-chosen
// for that M (same column padding), the K slicing KEPT.  An output element's value depends only on the slicing of K and on
// the fixed chunk-by-chunk MFMA chain, not on the tile shape, so every frame of the group gets the bits of a single enqueue.
static std::vector<Conv> batch_plan(const std::vector<Conv>& single, int n, const PlanRule& p) {
  std::vector<Conv> out = single;
  if (n == 1) return out;
  for (Conv& c : out) {
    c.M = n * c.out_h * c.out_w;
    const int cfg = pick_cfg(c, p);
    if (c.npad % kCfg[cfg].bn == 0) c.cfg = cfg;  // the weights are stored with the single-frame column padding
  }
  return out;
}

// Workspace offsets (in elements of esz bytes) of every activation for groups of up to `frames` frames; returns the
// workspace elements.
static size_t layout_acts(std::vector<Act>& acts, int frames, size_t esz) {
  const size_t al = 256 / esz;  // 256-byte aligned
  size_t off = 0;
  for (Act& a : acts) {
    a.off = off;
    off += ((size_t)frames * a.h * a.w * a.c + al - 1) / al * al;
  }
  return off;
}

static size_t partial_floats_of(const std::vector<Conv>& plan) {
  size_t pmax = 0;
  for (const Conv& c : plan)
    if (c.splits > 1 && (size_t)c.splits * c.M * c.npad > pmax) pmax = (size_t)c.splits * c.M * c.npad;
  return pmax;
}

// Host image of the device weight buffer: per conv wt [K][npad] (k = (ky ks + kx) Cin_stored + c), bias, scale, shift.
// BN folded in float64, rounded once: scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale.
static void fill_weights(const pt_denoiser* d, const std::map<std::string, Tensor>& t, std::vector<float>& w) {
  w.assign(d->w_floats, 0.0f);
  for (const Conv& c : d->convs) {
    float* wt = w.data() + c.w_off;
    float* bias = wt + (size_t)c.K * c.npad;
    float* scale = bias + c.npad;
    float* shift = scale + c.npad;
    // (torch conv name, BN name or "", first column)
    std::vector<std::pair<std::string, std::string>> parts;
    std::string base = c.name;
    if (base.find("conv1+res_conv") != std::string::npos) {
      const std::string blk = base.substr(0, base.find('.'));
      parts = {{blk + ".conv1", blk + ".bn1"}, {blk + ".res_conv", blk + ".res_bn"}};
    } else if (base.find(".conv2") != std::string::npos) {
      const std::string blk = base.substr(0, base.find('.'));
      parts = {{blk + ".conv2", blk + ".bn2"}};
    } else {
      parts = {{base, ""}};
    }
    int col = 0;
    for (const auto& pr : parts) {
      const Tensor& W = t.at(pr.first + ".weight");
      const Tensor& B = t.at(pr.first + ".bias");
      const int cout = (int)W.shape[0], cin = (int)W.shape[1], ks = (int)W.shape[2];
      for (int o = 0; o < cout; o++) {
        for (int ci = 0; ci < cin; ci++)
          for (int ky = 0; ky < ks; ky++)
            for (int kx = 0; kx < ks; kx++) {
              const size_t k = (size_t)(ky * ks + kx) * c.cin + ci;
              wt[k * c.npad + col + o] = ld_f32(W, ((size_t)(o * cin + ci) * ks + ky) * ks + kx);
            }
        bias[col + o] = ld_f32(B, o);
        if (pr.second.empty()) {
          scale[col + o] = 1.0f;
          shift[col + o] = 0.0f;
        } else {
          const double g = ld_f32(t.at(pr.second + ".weight"), o), be = ld_f32(t.at(pr.second + ".bias"), o);
          const double mu = ld_f32(t.at(pr.second + ".running_mean"), o), var = ld_f32(t.at(pr.second + ".running_var"), o);
          const double s = g / sqrt(var + 1e-5);
          scale[col + o] = (float)s;
          shift[col + o] = (float)(be - mu * s);
        }
      }
      col += cout;
    }
  }
}

static const std::vector<Conv>& plan_for(pt_denoiser* d, int n) {
  if (n == 1) return d->convs;
  auto it = d->plans.find(n);
  if (it == d->plans.end()) it = d->plans.emplace(n, batch_plan(d->convs, n, kPlan[d->precision])).first;
  return it->second;
}

// The kernel arguments of one conv for a denoiser that stores T: activations and weights of T, fp32 bias / scale / shift
// and split-K partials, the head's output in fp32.
template <class T>
static ConvArgs<T> conv_args(const pt_denoiser* d, const Conv& c, float* frame_out, int frame_ld, size_t frame_stride, int frames) {
  ConvArgs<T> a{};
  T* ws = reinterpret_cast<T*>(d->d_ws);
  a.in = ws + d->acts[c.in].off;
  a.in_h = c.in_h, a.in_w = c.in_w, a.cin = c.cin;
  if constexpr (std::is_same<T, float>::value)
    a.wt = d->d_w + c.w_off;
  else
    a.wt = d->d_wh + c.h_off;
  a.npad = c.npad, a.ks = c.ks, a.stride = c.stride;
  a.out_w = c.out_w, a.out_h = c.out_h, a.M = c.M, a.N = c.N;
  a.nchunks = c.nchunks, a.chunks_per_split = c.chunks_per_split;
  a.partial = c.splits > 1 ? d->d_partial : nullptr;
  a.epi = c.epi;
  a.bias = d->d_w + c.p_off;
  a.scale = a.bias + c.npad;
  a.shift = a.scale + c.npad;
  if (c.out0 >= 0) {
    a.out0 = ws + d->acts[c.out0].off;
    a.ld0 = d->acts[c.out0].c;
  } else {
    a.rgb = frame_out;
    if constexpr (std::is_same<T, float>::value) a.out0 = frame_out;  // head_out
    a.ld0 = frame_ld;
  }
  a.nsplit = c.nsplit;
  if (c.out1 >= 0) {
    a.out1 = ws + d->acts[c.out1].off;
    a.ld1 = d->acts[c.out1].c;
  }
  if (c.res >= 0) a.res = ws + d->acts[c.res].off;
  if (c.up >= 0) {
    a.up = ws + d->acts[c.up].off;
    a.up_h = d->acts[c.up].h, a.up_w = d->acts[c.up].w;
  }
  a.x0 = ws + d->acts[0].off;
  a.frames = frames, a.out_hw = c.out_h * c.out_w;
  a.frame_stride = frame_stride;
  return a;
}

template <class T>
static int launch_conv_t(const pt_denoiser* d, const Conv& c, float* frame_out, int frame_ld, size_t frame_stride, int frames,
                         hipStream_t s, int* launches) {
  const dim3 grid((c.M + kCfg[c.cfg].bm - 1) / kCfg[c.cfg].bm, c.npad / kCfg[c.cfg].bn, c.splits);
  const ConvArgs<T> a = conv_args<T>(d, c, frame_out, frame_ld, frame_stride, frames);
  switch (c.cfg) {
    case 0: hipLaunchKernelGGL((conv_kernel<T, 2, 1, 4, 1>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((conv_kernel<T, 1, 2, 4, 1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((conv_kernel<T, 2, 2, 2, 2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((conv_kernel<T, 1, 1, 4, 1>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((conv_kernel<T, 1, 1, 2, 2>), grid, dim3(256), 0, s, a); break;
  }
  PT_HIP(hipGetLastError());
  (*launches)++;
  if (c.splits > 1) {
    const uint32_t n = (uint32_t)c.M * (uint32_t)c.N;
    hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, s, a, c.splits);
    PT_HIP(hipGetLastError());
    (*launches)++;
  }
  return PT_OK;
}

// One conv of a group of `frames` frames (c from that group size's plan): its GEMM and, split, its reduction.
static int launch_conv(const pt_denoiser* d, const Conv& c, float* frame_out, int frame_ld, size_t frame_stride, int frames,
                       hipStream_t s, int* launches) {
  if (c.epi != EPI_ACT && kCfg[c.cfg].bn != 32)
    return pt_fail(PT_EINVAL, "launch_conv: %s: the lateral and head epilogues need 32-column tiles", c.name.c_str());
  return d->precision == PT_DENOISE_F16 ? launch_conv_t<_Float16>(d, c, frame_out, frame_ld, frame_stride, frames, s, launches)
                                        : launch_conv_t<float>(d, c, frame_out, frame_ld, frame_stride, frames, s, launches);
}

// The pre-processing of a group of g frames: the channel maxima, then the divisions and the stored copy x0.
template <class T>
static int launch_pre(const pt_denoiser* d, float* frames, size_t frame_stride, uint32_t pixels, int g, int inplace, hipStream_t s) {
  T* x0 = reinterpret_cast<T*>(d->d_ws) + d->acts[0].off;
  hipLaunchKernelGGL(pre_max_kernel, dim3(d->pre_blocks, g), dim3(256), 0, s, frames, frame_stride, pixels, d->d_premax);
  PT_HIP(hipGetLastError());
  hipLaunchKernelGGL(pre_apply_kernel<T>, dim3((pixels + 255) / 256, g), dim3(256), 0, s, frames, frame_stride, pixels, d->d_premax,
                     d->pre_blocks, x0, inplace);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

#if PT_BUILD_EXPERIMENTS
// Lab accessors: the host sees float32 in both modes (every half is one exactly); what it sets is rounded to nearest even,
// saturating like every store of the half mode.
template <class T>
static int copy_out(const pt_denoiser* d, const Act& a, float* h_out, size_t n) {
  std::vector<T> tmp(n);
  PT_HIP(hipMemcpy(tmp.data(), d->d_ws + a.off * sizeof(T), n * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) h_out[i] = (float)tmp[i];
  return PT_OK;
}
template <class T>
static int copy_in(const pt_denoiser* d, const Act& a, const float* h_in, size_t n) {
  std::vector<T> tmp(n);
  for (size_t i = 0; i < n; i++)
    tmp[i] = std::is_same<T, float>::value ? (T)h_in[i] : (T)fminf(fmaxf(h_in[i], -HALF_MAX), HALF_MAX);
  PT_HIP(hipMemcpy(d->d_ws + a.off * sizeof(T), tmp.data(), n * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}
#endif

extern "C" {

int pt_denoiser_weights_check(const void* blob, size_t bytes) {
  return parse_weights(blob, bytes, nullptr, "pt_denoiser_weights_check");
}

int pt_denoiser_destroy(pt_denoiser* d) {
  if (!d) return PT_OK;
  if (d->d_w) (void)hipFree(d->d_w);
  if (d->d_wh) (void)hipFree(d->d_wh);
  if (d->d_ws) (void)hipFree(d->d_ws);
  if (d->d_partial) (void)hipFree(d->d_partial);
  if (d->d_premax) (void)hipFree(d->d_premax);
  pt_stage::destroy_events(d);
  delete d;
  return PT_OK;
}

// Half mode: every convolution weight must be representable (the conversion rounds to nearest even; it does not saturate).
static int check_half_range(const std::map<std::string, Tensor>& t, const char* who) {
  for (const auto& kv : t) {
    if (kv.second.shape.size() != 4) continue;  // convolution weights; bias and batch-norm tensors stay fp32
    for (size_t i = 0; i < kv.second.count; i++) {
      const float v = ld_f32(kv.second, i);
      if (fabsf(v) > HALF_MAX)
        return pt_fail(PT_EINVAL, "%s: tensor '%s' holds %g at element %zu: outside the fp16 range of +-65504 (PT_DENOISE_F16)", who,
                       kv.first.c_str(), (double)v, i);
    }
  }
  return PT_OK;
}

// The half image of the convolution weights: each conv's [K][npad] floats re-laid out as [K / 8][npad][8] halves (a lane's
// B fragment, 8 consecutive k of one column, is 16 contiguous bytes), rounded to nearest even; and the packed parameters.
static void half_weights(const pt_denoiser* d, const std::vector<float>& w, std::vector<_Float16>& wh, std::vector<float>& wp) {
  wh.assign(d->wh_halves, (_Float16)0.0f);
  wp.assign(d->p_floats, 0.0f);
  for (const Conv& c : d->convs) {
    const float* wt = w.data() + c.w_off;
    _Float16* o = wh.data() + c.h_off;
    for (int k = 0; k < c.K; k++)
      for (int n = 0; n < c.npad; n++) o[((size_t)(k >> 3) * c.npad + n) * 8 + (k & 7)] = (_Float16)wt[(size_t)k * c.npad + n];
    memcpy(wp.data() + c.p_off, wt + (size_t)c.K * c.npad, 3 * (size_t)c.npad * sizeof(float));
  }
}

int pt_denoiser_create_opts(int width, int height, const void* blob, size_t bytes, const pt_denoiser_opts* opts, pt_denoiser** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_denoiser_create: null output pointer");
  *out = nullptr;
  if (!opts) return pt_fail(PT_EINVAL, "pt_denoiser_create_opts: null options");
  if (opts->precision != PT_DENOISE_F32 && opts->precision != PT_DENOISE_F16)
    return pt_fail(PT_EINVAL, "pt_denoiser_create_opts: precision %d is neither PT_DENOISE_F32 (0) nor PT_DENOISE_F16 (1)", opts->precision);
  if (opts->max_frames < 1) return pt_fail(PT_EINVAL, "pt_denoiser_create_opts: max_frames %d < 1", opts->max_frames);
  for (int i = 0; i < 6; i++)
    if (opts->reserved[i] != 0) return pt_fail(PT_EINVAL, "pt_denoiser_create_opts: reserved[%d] = %d must be 0", i, opts->reserved[i]);
  if (width <= 0 || height <= 0 || (int64_t)width * height > 4096 * 4096)
    return pt_fail(PT_EINVAL, "pt_denoiser_create: frame size %d x %d outside 1 .. 4096 x 4096 pixels", width, height);
  int rc = pt_stage::check_batch("pt_denoiser_create_opts", opts->max_frames, width, height);
  if (rc != PT_OK) return rc;
  std::map<std::string, Tensor> t;
  if ((rc = parse_weights(blob, bytes, &t, "pt_denoiser_create")) != PT_OK) return rc;
  const bool half = opts->precision == PT_DENOISE_F16;
  if (half && (rc = check_half_range(t, "pt_denoiser_create_opts")) != PT_OK) return rc;
  if ((rc = pt_stage::check_device("pt_denoiser_create")) != PT_OK) return rc;
  pt_denoiser* d = new (std::nothrow) pt_denoiser();
  if (!d) return pt_fail(PT_ENOMEM, "pt_denoiser_create: out of host memory");
  d->width = width, d->height = height;
  d->precision = opts->precision;
  d->esz = half ? sizeof(_Float16) : sizeof(float);
  build_layers(d);
  d->ws_elems = layout_acts(d->acts, 1, d->esz);
  d->partial_floats = partial_floats_of(d->convs);
  std::vector<float> w, wp;
  std::vector<_Float16> wh;
  fill_weights(d, t, w);
  if (half) half_weights(d, w, wh, wp);
  const std::vector<float>& wf = half ? wp : w;  // what d_w holds
  d->pre_blocks = (int)(((uint64_t)width * height + 255) / 256);
  if (d->pre_blocks > PRE_BLOCKS) d->pre_blocks = PRE_BLOCKS;
  hipError_t e = hipGetDevice(&d->device);
  if (e == hipSuccess) e = hipMalloc((void**)&d->d_w, wf.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d->d_w, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && half) e = hipMalloc((void**)&d->d_wh, wh.size() * sizeof(_Float16));
  if (e == hipSuccess && half) e = hipMemcpy(d->d_wh, wh.data(), wh.size() * sizeof(_Float16), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&d->d_ws, d->ws_elems * d->esz);
  if (e == hipSuccess) e = hipMemset(d->d_ws, 0, d->ws_elems * d->esz);
  if (e == hipSuccess && d->partial_floats) e = hipMalloc((void**)&d->d_partial, d->partial_floats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d->d_premax, PRE_BLOCKS * 5 * sizeof(float));
  if ((rc = pt_stage::create_events("pt_denoiser_create", e, d, pt_denoiser_destroy)) != PT_OK) return rc;
  if (opts->max_frames > 1 && (rc = pt_denoiser_reserve_frames(d, opts->max_frames)) != PT_OK) {
    pt_denoiser_destroy(d);
    return rc;
  }
  *out = d;
  return PT_OK;
}

int pt_denoiser_create(int width, int height, const void* blob, size_t bytes, pt_denoiser** out) {
  pt_denoiser_opts opts{};
  opts.precision = PT_DENOISE_F32, opts.max_frames = 1;
  return pt_denoiser_create_opts(width, height, blob, bytes, &opts, out);
}

int pt_denoiser_create_opts_from_file(int width, int height, const char* path, const pt_denoiser_opts* opts, pt_denoiser** out) {
  if (!path) return pt_fail(PT_EINVAL, "pt_denoiser_create_from_file: null path");
  FILE* f = fopen(path, "rb");
  if (!f) return pt_fail(PT_EINVAL, "pt_denoiser_create_from_file: cannot open '%s'", path);
  std::vector<unsigned char> buf;
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  return pt_denoiser_create_opts(width, height, buf.data(), buf.size(), opts, out);
}

int pt_denoiser_create_from_file(int width, int height, const char* path, pt_denoiser** out) {
  pt_denoiser_opts opts{};
  opts.precision = PT_DENOISE_F32, opts.max_frames = 1;
  return pt_denoiser_create_opts_from_file(width, height, path, &opts, out);
}

int pt_denoiser_precision(const pt_denoiser* d, int* out) {
  if (!d || !out) return pt_fail(PT_EINVAL, "pt_denoiser_precision: null %s", d ? "output pointer" : "denoiser");
  *out = d->precision;
  return PT_OK;
}

int pt_denoiser_reserve_frames(pt_denoiser* d, int max_frames) {
  if (!d) return pt_fail(PT_EINVAL, "pt_denoiser_reserve_frames: null denoiser");
  if (max_frames < 1) return pt_fail(PT_EINVAL, "pt_denoiser_reserve_frames: max_frames %d < 1", max_frames);
  if (max_frames <= d->max_frames) return PT_OK;
  int rc = pt_stage::check_batch("pt_denoiser_reserve_frames", max_frames, d->width, d->height);
  if (rc != PT_OK) return rc;
  const std::vector<Conv> plan = batch_plan(d->convs, max_frames, kPlan[d->precision]);
  for (const Conv& c : plan)  // splitk_reduce_kernel indexes M x N elements in 32 bits
    if ((int64_t)c.M * c.N > (int64_t)UINT32_MAX)
      return pt_fail(PT_EINVAL, "pt_denoiser_reserve_frames: max_frames %d: layer %s has too many elements", max_frames, c.name.c_str());
  std::vector<Act> acts = d->acts;
  const size_t ws_elems = layout_acts(acts, max_frames, d->esz);
  const size_t partial_floats = partial_floats_of(plan);
  const pt_stage::Buffer bufs[3] = {{(void**)&d->d_ws, ws_elems * d->esz, true},
                                    {(void**)&d->d_partial, partial_floats * sizeof(float), false},
                                    {(void**)&d->d_premax, (size_t)max_frames * PRE_BLOCKS * 5 * sizeof(float), false}};
  rc = pt_stage::grow_workspace("pt_denoiser_reserve_frames", bufs, "%d frames (%zu + %zu workspace elements)", max_frames, ws_elems,
                                partial_floats);
  if (rc != PT_OK) return rc;
  d->acts = acts;
  d->ws_elems = ws_elems, d->partial_floats = partial_floats;
  d->max_frames = max_frames;
  return PT_OK;
}

// (every check before any launch: a refused call launches nothing, and the lab counters say so.  The timed call refuses in the
// words of the call it wraps.)
static int check_frames_args(pt_denoiser* d, int n_frames, const float* d_frames, size_t frame_stride_floats, const float* d_rgb,
                             size_t rgb_stride_floats) {
  d->last_groups = d->last_launches = 0;
  if (!d_frames) return pt_fail(PT_EINVAL, "pt_denoiser_enqueue_frames: null d_frames");
  if (n_frames < 1) return pt_fail(PT_EINVAL, "pt_denoiser_enqueue_frames: n_frames %d < 1", n_frames);
  const size_t pixels = (size_t)d->width * d->height;
  if (frame_stride_floats < pixels * 14)
    return pt_fail(PT_EINVAL, "pt_denoiser_enqueue_frames: frame_stride_floats %zu < width x height x 14 = %zu", frame_stride_floats,
                   pixels * 14);
  if (d_rgb && rgb_stride_floats < pixels * 3)
    return pt_fail(PT_EINVAL, "pt_denoiser_enqueue_frames: rgb_stride_floats %zu < width x height x 3 = %zu", rgb_stride_floats, pixels * 3);
  return PT_OK;
}

int pt_denoiser_enqueue_frames(pt_denoiser* d, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                               size_t rgb_stride_floats, void* hip_stream) {
  if (!d) return pt_fail(PT_EINVAL, "pt_denoiser_enqueue_frames: null denoiser");
  int rc = check_frames_args(d, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats);
  if (rc != PT_OK) return rc;
  const uint32_t pixels = (uint32_t)d->width * (uint32_t)d->height;
  hipStream_t s = (hipStream_t)hip_stream;
  for (int f0 = 0; f0 < n_frames; f0 += d->max_frames) {
    const int g = n_frames - f0 < d->max_frames ? n_frames - f0 : d->max_frames;
    float* frames = d_frames + (size_t)f0 * frame_stride_floats;
    float* out = d_rgb ? d_rgb + (size_t)f0 * rgb_stride_floats : frames;
    rc = d->precision == PT_DENOISE_F16 ? launch_pre<_Float16>(d, frames, frame_stride_floats, pixels, g, d_rgb ? 0 : 1, s)
                                        : launch_pre<float>(d, frames, frame_stride_floats, pixels, g, d_rgb ? 0 : 1, s);
    if (rc != PT_OK) return rc;
    d->last_launches += 2;
    for (const Conv& c : plan_for(d, g)) {
      rc = launch_conv(d, c, out, d_rgb ? 3 : 14, d_rgb ? rgb_stride_floats : frame_stride_floats, g, s, &d->last_launches);
      if (rc != PT_OK) return rc;
    }
    d->last_groups++;
  }
  return PT_OK;
}

// One frame = a group of one: the single-frame table, the launches and the bits of the original single-frame path.
int pt_denoiser_enqueue(pt_denoiser* d, float* d_frame, float* d_rgb, void* hip_stream) {
  if (!d || !d_frame) return pt_fail(PT_EINVAL, "pt_denoiser_enqueue: null denoiser or frame");
  const size_t pixels = (size_t)d->width * d->height;
  return pt_denoiser_enqueue_frames(d, 1, d_frame, pixels * 14, d_rgb, pixels * 3, hip_stream);
}

int pt_denoiser_denoise_frames(pt_denoiser* d, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                               size_t rgb_stride_floats, float* ms_out) {
  if (!d) return pt_fail(PT_EINVAL, "pt_denoiser_denoise_frames: null denoiser");
  const int rc = check_frames_args(d, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats);
  if (rc != PT_OK) return rc;
  return pt_stage::run_timed(d->ev0, d->ev1, ms_out, [&] {
    return pt_denoiser_enqueue_frames(d, n_frames, d_frames, frame_stride_floats, d_rgb, rgb_stride_floats, nullptr);
  });
}

int pt_denoiser_denoise(pt_denoiser* d, float* d_frame, float* d_rgb, float* ms_out) {
  if (!d) return pt_fail(PT_EINVAL, "pt_denoiser_denoise: null denoiser");
  if (!d_frame) return pt_fail(PT_EINVAL, "pt_denoiser_enqueue: null denoiser or frame");
  const size_t pixels = (size_t)d->width * d->height;
  return pt_denoiser_denoise_frames(d, 1, d_frame, pixels * 14, d_rgb, pixels * 3, ms_out);
}

#if PT_BUILD_EXPERIMENTS
int pt_debug_denoiser_layer_info(pt_denoiser* d, int layer, int* n_layers, int shape[3], char* name, size_t name_len) {
  if (!d) return pt_fail(PT_EINVAL, "pt_debug_denoiser_layer_info: null denoiser");
  if (n_layers) *n_layers = (int)d->acts.size();
  if (layer < 0 || layer >= (int)d->acts.size()) return pt_fail(PT_EINVAL, "pt_debug_denoiser_layer_info: no layer %d", layer);
  const Act& a = d->acts[layer];
  if (shape) shape[0] = a.h, shape[1] = a.w, shape[2] = a.c;
  if (name && name_len) snprintf(name, name_len, "%s", a.name.c_str());
  return PT_OK;
}

// The group hooks take 1 .. max_frames frames: what the workspace was laid out for.
static int check_group(const pt_denoiser* d, int frames, const char* who) {
  if (frames < 1 || frames > d->max_frames)
    return pt_fail(PT_EINVAL, "%s: frames %d outside 1 .. max_frames = %d", who, frames, d->max_frames);
  return PT_OK;
}

// (the first `frames` frames of an activation laid out for max_frames are contiguous from its offset)
int pt_debug_denoiser_activation_frames(pt_denoiser* d, int layer, int frames, float* h_out, size_t n_floats) {
  if (!d || !h_out || layer < 0 || layer >= (int)d->acts.size())
    return pt_fail(PT_EINVAL, "pt_debug_denoiser_activation: bad arguments");
  const int rc = check_group(d, frames, "pt_debug_denoiser_activation");
  if (rc != PT_OK) return rc;
  const Act& a = d->acts[layer];
  const size_t n = (size_t)frames * a.h * a.w * a.c;
  if (n_floats != n) return pt_fail(PT_EINVAL, "pt_debug_denoiser_activation: layer %d holds %zu floats, not %zu", layer, n, n_floats);
  PT_HIP(hipDeviceSynchronize());
  return d->precision == PT_DENOISE_F16 ? copy_out<_Float16>(d, a, h_out, n) : copy_out<float>(d, a, h_out, n);
}

int pt_debug_denoiser_activation(pt_denoiser* d, int layer, float* h_out, size_t n_floats) {
  return pt_debug_denoiser_activation_frames(d, layer, 1, h_out, n_floats);
}

int pt_debug_denoiser_set_activation_frames(pt_denoiser* d, int layer, int frames, const float* h_in, size_t n_floats) {
  if (!d || !h_in || layer < 0 || layer >= (int)d->acts.size())
    return pt_fail(PT_EINVAL, "pt_debug_denoiser_set_activation: bad arguments");
  const int rc = check_group(d, frames, "pt_debug_denoiser_set_activation");
  if (rc != PT_OK) return rc;
  const Act& a = d->acts[layer];
  const size_t n = (size_t)frames * a.h * a.w * a.c;
  if (n_floats != n) return pt_fail(PT_EINVAL, "pt_debug_denoiser_set_activation: layer %d holds %zu floats, not %zu", layer, n, n_floats);
  PT_HIP(hipDeviceSynchronize());
  return d->precision == PT_DENOISE_F16 ? copy_in<_Float16>(d, a, h_in, n) : copy_in<float>(d, a, h_in, n);
}

int pt_debug_denoiser_set_activation(pt_denoiser* d, int layer, const float* h_in, size_t n_floats) {
  return pt_debug_denoiser_set_activation_frames(d, layer, 1, h_in, n_floats);
}

int pt_debug_denoiser_conv_info(pt_denoiser* d, int conv, int* n_convs, int info[12], char* name, size_t name_len) {
  if (!d) return pt_fail(PT_EINVAL, "pt_debug_denoiser_conv_info: null denoiser");
  if (n_convs) *n_convs = (int)d->convs.size();
  if (conv < 0 || conv >= (int)d->convs.size()) return pt_fail(PT_EINVAL, "pt_debug_denoiser_conv_info: no conv %d", conv);
  const Conv& c = d->convs[conv];
  if (info) {
    const int v[12] = {c.in, c.out0, c.out1, c.res, c.up, c.ks, c.stride, c.N, c.epi, c.splits, kCfg[c.cfg].bm, kCfg[c.cfg].bn};
    memcpy(info, v, sizeof(v));
  }
  if (name && name_len) snprintf(name, name_len, "%s", c.name.c_str());
  return PT_OK;
}

int pt_debug_denoiser_run_conv_frames(pt_denoiser* d, int conv, float* d_out, int frames, int ld, size_t frame_stride) {
  if (!d || conv < 0 || conv >= (int)d->convs.size()) return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_conv: bad arguments");
  int rc = check_group(d, frames, "pt_debug_denoiser_run_conv");
  if (rc != PT_OK) return rc;
  const Conv& c = plan_for(d, frames)[conv];
  if (c.out0 < 0) {  // the head writes d_out + f * frame_stride + pixel * ld + (0 .. 2)
    if (!d_out) return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_conv: the rgb head needs an output buffer");
    const size_t pixels = (size_t)d->width * d->height;
    if (ld < 3) return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_conv: ld %d < 3", ld);
    if (frame_stride < pixels * (size_t)ld)
      return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_conv: frame_stride %zu < width x height x ld = %zu", frame_stride, pixels * (size_t)ld);
  }
  int launches = 0;
  rc = launch_conv(d, c, d_out, ld, frame_stride, frames, nullptr, &launches);
  if (rc != PT_OK) return rc;
  PT_HIP(hipDeviceSynchronize());
  return PT_OK;
}

int pt_debug_denoiser_run_conv(pt_denoiser* d, int conv, float* d_rgb) {
  if (!d) return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_conv: bad arguments");
  return pt_debug_denoiser_run_conv_frames(d, conv, d_rgb, 1, 3, (size_t)d->width * d->height * 3);
}

int pt_debug_denoiser_run_pre(pt_denoiser* d, float* d_frames, int frames, size_t frame_stride, int inplace) {
  if (!d || !d_frames) return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_pre: null denoiser or frames");
  const int rc0 = check_group(d, frames, "pt_debug_denoiser_run_pre");
  if (rc0 != PT_OK) return rc0;
  const uint32_t pixels = (uint32_t)d->width * (uint32_t)d->height;
  if (frame_stride < (size_t)pixels * 14)
    return pt_fail(PT_EINVAL, "pt_debug_denoiser_run_pre: frame_stride %zu < width x height x 14 = %zu", frame_stride, (size_t)pixels * 14);
  const int rc = d->precision == PT_DENOISE_F16 ? launch_pre<_Float16>(d, d_frames, frame_stride, pixels, frames, inplace ? 1 : 0, nullptr)
                                                : launch_pre<float>(d, d_frames, frame_stride, pixels, frames, inplace ? 1 : 0, nullptr);
  if (rc != PT_OK) return rc;
  PT_HIP(hipDeviceSynchronize());
  return PT_OK;
}

int pt_debug_denoiser_memory(pt_denoiser* d, int layer, uint64_t info[6]) {
  if (!d || !info) return pt_fail(PT_EINVAL, "pt_debug_denoiser_memory: null denoiser or output");
  if (layer < 0 || layer >= (int)d->acts.size()) return pt_fail(PT_EINVAL, "pt_debug_denoiser_memory: no layer %d", layer);
  const Act& a = d->acts[layer];
  info[0] = d->esz;
  info[1] = a.off * d->esz;
  info[2] = (uint64_t)a.h * a.w * a.c * d->esz;
  info[3] = d->ws_elems * d->esz;
  info[4] = d->partial_floats * sizeof(float);
  info[5] = d->precision == PT_DENOISE_F16 ? d->wh_halves * sizeof(_Float16) + d->p_floats * sizeof(float) : d->w_floats * sizeof(float);
  return PT_OK;
}

int pt_debug_denoiser_last_enqueue(pt_denoiser* d, int* groups, int* launches) {
  if (!d) return pt_fail(PT_EINVAL, "pt_debug_denoiser_last_enqueue: null denoiser");
  if (groups) *groups = d->last_groups;
  if (launches) *launches = d->last_launches;
  return PT_OK;
}

int pt_debug_denoiser_conv_plan(pt_denoiser* d, int n_frames, int conv, int info[6]) {
  if (!d) return pt_fail(PT_EINVAL, "pt_debug_denoiser_conv_plan: null denoiser");
  if (n_frames < 1 || n_frames > pt_stage::MAX_FRAMES || (int64_t)n_frames * d->width * d->height > pt_stage::MAX_BATCH_PIXELS)
    return pt_fail(PT_EINVAL, "pt_debug_denoiser_conv_plan: n_frames %d outside the batch limits", n_frames);
  if (conv < 0 || conv >= (int)d->convs.size()) return pt_fail(PT_EINVAL, "pt_debug_denoiser_conv_plan: no conv %d", conv);
  const Conv& c = plan_for(d, n_frames)[conv];
  if (info) {
    const int64_t wg = (int64_t)((c.M + kCfg[c.cfg].bm - 1) / kCfg[c.cfg].bm) * (c.npad / kCfg[c.cfg].bn) * c.splits;
    const int v[6] = {c.M, kCfg[c.cfg].bm, kCfg[c.cfg].bn, c.splits, c.chunks_per_split, (int)wg};
    memcpy(info, v, sizeof(v));
  }
  return PT_OK;
}
#endif

}  // extern "C"
