// pt_patches.hip -- the training-patch session behind pt_patches_* (include/ptcore.h): from a (train frame, target image) pair on
// the device, the pre-processed [N][14][P][P] inputs and the clamped [N][3][P][P] targets that a CNN's data loader consumes, and
// the score by which the reference picks its patches (load_data.py: get_score, the pooled variance of the pre-processed colour
// plus that of the normal) as integer sums that are exact in any order.  The pre-processing is the network's own
// (pt_denoise.hip: pre_max_kernel, pre_apply_kernel), restated here and held to the same bits.  DENOISER.md, "Training
// patches", states the definition; tests/patches_model.py restates it in NumPy.  EXACT code, like pt_tonemap.hip and
// pt_compare.hip: no contraction, IEEE divisions, no transcendental on the device.
//
// Four kernels.  max: per-workgroup maxima of channels 9-13 of the frame (prepare); whoever divides folds them.  score: blockIdx.y
// = patch, a workgroup walks 1024 of the patch's pixels and writes its eight sums; sum: one workgroup per patch adds them into
// the patch's record.  gather: blockIdx.y = patch, a workgroup stages runs of up to 128 pixels of a patch row (and the target's
// colour) in LDS, read as contiguous floats, and writes each of the 17 planes' pieces as aligned 16-byte stores with scalar
// heads and tails.  No atomics, no memset, no host synchronisation.  Corners are checked on the host before anything is
// launched: no kernel is handed an address that was not proven to lie inside the caller's images.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "pt_stage.h"
#include "pt_stage_device.h"

namespace ptpat {

constexpr int BLOCK = 256;          // lanes per workgroup of every kernel
constexpr int MAX_PARTS = BLOCK;    // workgroups of the maxima kernel: one lane of a consumer folds one of them
constexpr int SCORE_PIXELS = 1024;  // pixels of a patch per score workgroup
constexpr int RUN = 128;            // pixels of a patch row per staging of the gather
constexpr int VECS = RUN / 4;       // 16-byte pieces of a run
constexpr int SLOTS = VECS + 2;     // ... plus its scalar head and tail
constexpr int PLANES = 14 + 3;      // the staged rows: a pixel's 14 channels and the target's colour
// Row pitch of the staging array in floats.  The staging writes channel c of pixel e to row c, column e from lanes that walk
// (e, c) with c fastest: bank (3 c + e) mod 32 is distinct for the (c, e) pairs of a 32-lane half but for a wrap.
constexpr int PITCH = RUN + 3;
constexpr int RING = 4;             // pinned staging slots of the corners
constexpr float EPS = 0.00316f, X_MAX = 65504.0f;
constexpr double Q = 1048576.0;     // 2^20

struct Sums {  // of one population pair: {S1, A, B, C} of the colour, then of the normal
  uint64_t v[8];
};

struct Corner {
  int32_t x, y;
};

#pragma clang fp contract(off)

__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* red) { return pt_stage::block_sum<BLOCK>(v, red); }

// every lane's mx[k] = the maximum over its wave; lane 0 of each wave leaves it in wmx (the caller's barrier follows)
__device__ __forceinline__ void wave_max5(float (&mx)[5], float (*wmx)[5]) {
#pragma unroll
  for (int k = 0; k < 5; k++)
    for (int s = 1; s < 64; s <<= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], s));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 5; k++) wmx[wave][k] = mx[k];
}

__device__ __forceinline__ float fold4(float (*wmx)[5], int k) { return fmaxf(fmaxf(wmx[0][k], wmx[1][k]), fmaxf(wmx[2][k], wmx[3][k])); }

// Step 1, first half: part[block][5] = maxima of channels 9-13 over the block's pixels (a max is exact in any order; fmaxf
// from -inf ignores NaNs).  The shape of pt_denoise.hip's pre_max_kernel.
__global__ void __launch_bounds__(BLOCK) max_kernel(const float* __restrict__ frame, uint32_t pixels, float* __restrict__ part) {
  __shared__ float wmx[BLOCK / 64][5];
  float mx[5];
#pragma unroll
  for (int k = 0; k < 5; k++) mx[k] = -INFINITY;
  for (uint32_t p = blockIdx.x * (uint32_t)BLOCK + threadIdx.x; p < pixels; p += gridDim.x * (uint32_t)BLOCK)
#pragma unroll
    for (int k = 0; k < 5; k++) mx[k] = fmaxf(mx[k], frame[(size_t)p * 14 + 9 + k]);
  wave_max5(mx, wmx);
  __syncthreads();
  if (threadIdx.x < 5) part[(size_t)blockIdx.x * 5 + threadIdx.x] = fold4(wmx, (int)threadIdx.x);
}

// one value of a population into its four sums
__device__ __forceinline__ void tally(uint64_t* s, float v) {
  const int64_t q = (int64_t)floor((double)v * Q);
  const uint64_t a = (uint64_t)(q < 0 ? -q : q), ah = a >> 18, al = a & 0x3FFFFull;
  s[0] += (uint64_t)q;  // (wraps as two's complement)
  s[1] += ah * ah;
  s[2] += ah * al;
  s[3] += al * al;
}

// Step 3: partials[patch][chunk] = the eight sums over the chunk's pixels of the patch.  Every workgroup writes its record.
__global__ void __launch_bounds__(BLOCK) score_kernel(const float* __restrict__ train, int width, int patch, const Corner* __restrict__ corners,
                                                     uint32_t chunks, Sums* __restrict__ partials) {
  __shared__ uint64_t red[BLOCK / 64];
  const Corner c = corners[blockIdx.y];
  const uint32_t pp = (uint32_t)patch * (uint32_t)patch;
  const uint32_t first = blockIdx.x * (uint32_t)SCORE_PIXELS;
  const uint32_t last = first + SCORE_PIXELS < pp ? first + SCORE_PIXELS : pp;
  uint64_t s[8];
#pragma unroll
  for (int q = 0; q < 8; q++) s[q] = 0;
  for (uint32_t i = first + threadIdx.x; i < last; i += BLOCK) {
    const uint32_t j = i / (uint32_t)patch, x = i - j * (uint32_t)patch;
    const float* px = train + ((size_t)(c.y + (int)j) * (size_t)width + (size_t)(c.x + (int)x)) * 14;
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = px[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float t = v[k] / (EPS + v[6 + k]);
      t = t > 0.0f ? t : 0.0f;  // (NaN becomes 0)
      t = t < X_MAX ? t : X_MAX;
      tally(s, t);
      float n = v[3 + k];
      n = n == n ? n : 0.0f;
      n = n < X_MAX ? n : X_MAX;
      n = n > -X_MAX ? n : -X_MAX;
      tally(s + 4, n);
    }
  }
#pragma unroll
  for (int q = 0; q < 8; q++) s[q] = block_sum(s[q], red);
  if (threadIdx.x == 0) {
    Sums out;
#pragma unroll
    for (int q = 0; q < 8; q++) out.v[q] = s[q];
    partials[(size_t)blockIdx.y * chunks + blockIdx.x] = out;
  }
}

// One workgroup per patch: records[patch] = the sum of the patch's partials.
__global__ void __launch_bounds__(BLOCK) sum_kernel(const Sums* __restrict__ partials, uint32_t chunks, Sums* __restrict__ records) {
  __shared__ uint64_t red[BLOCK / 64];
  const Sums* p = partials + (size_t)blockIdx.x * chunks;
  uint64_t s[8];
#pragma unroll
  for (int q = 0; q < 8; q++) s[q] = 0;
  for (uint32_t b = threadIdx.x; b < chunks; b += BLOCK) {
    const Sums v = p[b];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] += v.v[q];
  }
#pragma unroll
  for (int q = 0; q < 8; q++) s[q] = block_sum(s[q], red);
  if (threadIdx.x == 0) {
    Sums out;
#pragma unroll
    for (int q = 0; q < 8; q++) out.v[q] = s[q];
    records[blockIdx.x] = out;
  }
}

struct Gather {
  const float* train;  // [height][width][14]
  const float* gt;     // [height][width][gt_stride]; unused without targets
  int gt_stride, width, patch;
  const Corner* corners;
  const float* part;  // [nparts][5]
  int nparts;
  float *inputs, *targets;  // targets may be null
  uint32_t runs, units;     // runs per patch row; rows x runs
};

// Steps 2 and 4.  A unit is a run of up to RUN pixels of one patch row: its 14 x len floats are contiguous in the frame and go
// to LDS as they lie; then plane c of the unit is len contiguous floats of the output, written as a scalar head up to the next
// 16-byte boundary, aligned 16-byte pieces, and a scalar tail (slot < VECS: piece, VECS: head, VECS + 1: tail).
__global__ void __launch_bounds__(BLOCK) gather_kernel(Gather a) {
  __shared__ float s[PLANES * PITCH];
  __shared__ float wmx[BLOCK / 64][5];
  __shared__ float s_div[5];
  {  // step 1, second half: fold the maxima, form the divisors
    float mx[5];
#pragma unroll
    for (int k = 0; k < 5; k++) mx[k] = (int)threadIdx.x < a.nparts ? a.part[(size_t)threadIdx.x * 5 + k] : -INFINITY;
    wave_max5(mx, wmx);
    __syncthreads();
    if (threadIdx.x < 5) s_div[threadIdx.x] = (float)(0.00316 + (double)fold4(wmx, (int)threadIdx.x));
  }  // (the barrier after the first staging publishes s_div)
  const uint32_t k = blockIdx.y;
  const Corner c = a.corners[k];
  const int P = a.patch;
  const int planes = a.targets ? PLANES : 14;
  for (uint32_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const uint32_t j = u / a.runs, r = u - j * a.runs;
    const int x0 = (int)r * RUN;
    const int len = P - x0 < RUN ? P - x0 : RUN;
    const size_t pix = (size_t)(c.y + (int)j) * (size_t)a.width + (size_t)(c.x + x0);
    const float* src = a.train + pix * 14;
    for (int f = threadIdx.x; f < len * 14; f += BLOCK) {
      const int e = f / 14, ch = f - e * 14;
      s[ch * PITCH + e] = src[f];
    }
    if (a.targets) {
      const float* g = a.gt + pix * (size_t)a.gt_stride;
      for (int f = threadIdx.x; f < len * 3; f += BLOCK) {
        const int e = f / 3, ch = f - e * 3;
        s[(14 + ch) * PITCH + e] = g[(size_t)e * (size_t)a.gt_stride + ch];
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < planes * SLOTS; t += BLOCK) {
      const int ch = t / SLOTS, slot = t - ch * SLOTS;
      float* dst = ch < 14 ? a.inputs + ((((size_t)k * 14 + ch) * P + j) * P + x0) : a.targets + ((((size_t)k * 3 + (ch - 14)) * P + j) * P + x0);
      int head = (int)((4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u);  // floats up to the next 16-byte boundary
      head = head < len ? head : len;
      const int nvec = (len - head) >> 2;
      int e0, cnt;
      if (slot < VECS) e0 = head + 4 * slot, cnt = slot < nvec ? 4 : 0;
      else if (slot == VECS) e0 = 0, cnt = head;
      else e0 = head + 4 * nvec, cnt = len - e0;
      if (cnt == 0) continue;
      const float* row = s + ch * PITCH + e0;
      const float* alb = s + (ch < 3 ? ch + 6 : ch) * PITCH + e0;  // (read for ch < 3 only)
      const float div = ch >= 9 && ch < 14 ? s_div[ch - 9] : 1.0f;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (i >= cnt) {
          v[i] = 0.0f;
          continue;
        }
        float x = row[i];
        if (ch < 3) x = x / (EPS + alb[i]);
        else if (ch >= 9 && ch < 14) x = x / div;
        else if (ch >= 14) {
          x = x > 0.0f ? x : 0.0f;  // (NaN becomes 0)
          x = x < 1.0f ? x : 1.0f;
        }
        v[i] = x;
      }
      if (slot < VECS) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        if (cnt > 0) dst[e0] = v[0];
        if (cnt > 1) dst[e0 + 1] = v[1];
        if (cnt > 2) dst[e0 + 2] = v[2];
      }
    }
    __syncthreads();  // (the next unit overwrites the staging array)
  }
}
}  // namespace ptpat

using namespace ptpat;

struct pt_patches {
  int width = 0, height = 0, patch = 0, max_patches = 0;
  uint32_t pixels = 0, nparts = 0, chunks = 0;  // workgroups of the maxima kernel; score workgroups per patch
  bool prepared = false;
  int last_patches = 0;             // patches of the last accepted score call: what pt_patches_result may ask for
  float* d_part = nullptr;          // [nparts][5]
  Corner* d_corners = nullptr;      // [max_patches]
  Sums* d_partials = nullptr;       // [max_patches][chunks]
  Sums* d_records = nullptr;        // [max_patches]
  Corner* h_corners = nullptr;      // pinned, [RING][max_patches]
  hipEvent_t slot_done[RING] = {};  // the copy out of a slot has run
  bool slot_used[RING] = {};
  int next_slot = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static size_t part_bytes(const pt_patches* s) { return (size_t)s->nparts * 5 * sizeof(float); }
static size_t corner_bytes(const pt_patches* s) { return (size_t)s->max_patches * sizeof(Corner); }
static size_t partial_bytes(const pt_patches* s) { return (size_t)s->max_patches * s->chunks * sizeof(Sums); }
static size_t record_bytes(const pt_patches* s) { return (size_t)s->max_patches * sizeof(Sums); }

// (every check before any launch: a refused call launches nothing and leaves the session and its results as they were)
static int check_corners(const char* who, const pt_patches* s, const float* d_train, int n, const int32_t* corners) {
  if (!d_train) return pt_fail(PT_EINVAL, "%s: null d_train", who);
  if (!s->prepared) return pt_fail(PT_EINVAL, "%s: no pt_patches_prepare before it: the divisors of the frame are not known", who);
  if (n < 1 || n > s->max_patches) return pt_fail(PT_EINVAL, "%s: n %d outside 1 .. max_patches = %d", who, n, s->max_patches);
  if (!corners) return pt_fail(PT_EINVAL, "%s: null corners", who);
  for (int k = 0; k < n; k++) {
    const int x = corners[2 * k], y = corners[2 * k + 1];
    if (x < 0 || x > s->width - s->patch)
      return pt_fail(PT_EINVAL, "%s: corners[%d].x = %d outside 0 .. width - patch = %d", who, k, x, s->width - s->patch);
    if (y < 0 || y > s->height - s->patch)
      return pt_fail(PT_EINVAL, "%s: corners[%d].y = %d outside 0 .. height - patch = %d", who, k, y, s->height - s->patch);
  }
  return PT_OK;
}

struct GatherCall {
  const float *d_train, *d_gt;
  int gt_pixel_stride, n;
  const int32_t* corners;
  float *d_inputs, *d_targets;
};

static int check_gather(const char* who, const pt_patches* s, const GatherCall& a) {
  if (!a.d_inputs) return pt_fail(PT_EINVAL, "%s: null d_inputs", who);
  if (a.d_targets) {
    if (!a.d_gt) return pt_fail(PT_EINVAL, "%s: null d_gt with d_targets given", who);
    if (a.gt_pixel_stride < 3 || a.gt_pixel_stride > 64)
      return pt_fail(PT_EINVAL, "%s: gt_pixel_stride %d outside 3 .. 64", who, a.gt_pixel_stride);
  }
  return check_corners(who, s, a.d_train, a.n, a.corners);
}

// The checked corners through a pinned slot to the device, on the call's stream.  A slot is written again only after the copy
// out of it has run (with RING slots in flight that wait has normally long passed).
static int stage_corners(pt_patches* s, int n, const int32_t* corners, hipStream_t st) {
  const int slot = s->next_slot;
  if (s->slot_used[slot]) PT_HIP(hipEventSynchronize(s->slot_done[slot]));
  Corner* h = s->h_corners + (size_t)slot * s->max_patches;
  memcpy(h, corners, (size_t)n * sizeof(Corner));
  PT_HIP(hipMemcpyAsync(s->d_corners, h, (size_t)n * sizeof(Corner), hipMemcpyHostToDevice, st));
  PT_HIP(hipEventRecord(s->slot_done[slot], st));
  s->slot_used[slot] = true;
  s->next_slot = (slot + 1) % RING;
  return PT_OK;
}

static int enqueue_prepare(pt_patches* s, const float* d_train, hipStream_t st) {
  hipLaunchKernelGGL(max_kernel, dim3(s->nparts), dim3(BLOCK), 0, st, d_train, s->pixels, s->d_part);
  PT_HIP(hipGetLastError());
  s->prepared = true;
  return PT_OK;
}

static int enqueue_score(pt_patches* s, const float* d_train, int n, const int32_t* corners, hipStream_t st) {
  const int rc = stage_corners(s, n, corners, st);
  if (rc != PT_OK) return rc;
  hipLaunchKernelGGL(score_kernel, dim3(s->chunks, (unsigned)n), dim3(BLOCK), 0, st, d_train, s->width, s->patch, (const Corner*)s->d_corners,
                     s->chunks, s->d_partials);
  PT_HIP(hipGetLastError());
  hipLaunchKernelGGL(sum_kernel, dim3((unsigned)n), dim3(BLOCK), 0, st, (const Sums*)s->d_partials, s->chunks, s->d_records);
  PT_HIP(hipGetLastError());
  s->last_patches = n;
  return PT_OK;
}

static int enqueue_gather(pt_patches* s, const GatherCall& a, hipStream_t st) {
  const int rc = stage_corners(s, a.n, a.corners, st);
  if (rc != PT_OK) return rc;
  Gather g{};
  g.train = a.d_train, g.gt = a.d_gt, g.gt_stride = a.gt_pixel_stride, g.width = s->width, g.patch = s->patch;
  g.corners = s->d_corners, g.part = s->d_part, g.nparts = (int)s->nparts;
  g.inputs = a.d_inputs, g.targets = a.d_targets;
  g.runs = (uint32_t)(s->patch + RUN - 1) / RUN;
  g.units = g.runs * (uint32_t)s->patch;
  const unsigned blocks = g.units < 256u ? g.units : 256u;
  hipLaunchKernelGGL(gather_kernel, dim3(blocks, (unsigned)a.n), dim3(BLOCK), 0, st, g);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// var = ((double)(N S2 - S1^2) / (double)(N N)) / 2^40 of one population, in 128-bit integers up to the one conversion
static double variance(const uint64_t* v, uint64_t values) {
  typedef unsigned __int128 u128;
  const __int128 s1 = (__int128)(int64_t)v[0];
  const u128 s2 = ((u128)v[1] << 36) + ((u128)v[2] << 19) + (u128)v[3];
  const u128 num = (u128)values * s2 - (u128)(s1 * s1);
  return ((double)num / (double)(values * values)) / 1099511627776.0;
}

extern "C" {

void pt_patches_opts_default(pt_patches_opts* opts) {
  if (!opts) return;
  *opts = pt_patches_opts{};
  opts->patch = 64;
  opts->max_patches = 64;
}

int pt_patches_destroy(pt_patches* s) {
  if (!s) return PT_OK;
  if (s->d_part) (void)hipFree(s->d_part);
  if (s->d_corners) (void)hipFree(s->d_corners);
  if (s->d_partials) (void)hipFree(s->d_partials);
  if (s->d_records) (void)hipFree(s->d_records);
  if (s->h_corners) (void)hipHostFree(s->h_corners);
  for (hipEvent_t e : s->slot_done)
    if (e) (void)hipEventDestroy(e);
  pt_stage::destroy_events(s);
  delete s;
  return PT_OK;
}

int pt_patches_create(int width, int height, const pt_patches_opts* opts, pt_patches** out) {
  const char* who = "pt_patches_create";
  if (!out) return pt_fail(PT_EINVAL, "%s: null output pointer", who);
  *out = nullptr;
  pt_patches_opts o;
  if (opts) o = *opts;
  else pt_patches_opts_default(&o);
  int rc = pt_stage::check_frame_size(who, width, height);
  if (rc != PT_OK) return rc;
  const int side = width < height ? width : height;
  const int most = side < 1024 ? side : 1024;
  if (o.patch < 1 || o.patch > most) return pt_fail(PT_EINVAL, "%s: patch %d outside 1 .. min(width, height, 1024) = %d", who, o.patch, most);
  if (o.max_patches < 1 || o.max_patches > pt_stage::MAX_FRAMES)
    return pt_fail(PT_EINVAL, "%s: max_patches %d outside 1 .. %d", who, o.max_patches, pt_stage::MAX_FRAMES);
  if ((int64_t)o.max_patches * o.patch * o.patch > pt_stage::MAX_BATCH_PIXELS)
    return pt_fail(PT_EINVAL, "%s: max_patches %d x patch %d x %d pixels exceeds the limit of %lld pixels", who, o.max_patches, o.patch, o.patch,
                   (long long)pt_stage::MAX_BATCH_PIXELS);
  for (int k = 0; k < 2; k++)
    if (o.reserved[k] != 0) return pt_fail(PT_EINVAL, "%s: reserved[%d] = %d must be 0", who, k, o.reserved[k]);
  if ((rc = pt_stage::check_device(who)) != PT_OK) return rc;
  pt_patches* s = new (std::nothrow) pt_patches();
  if (!s) return pt_fail(PT_ENOMEM, "%s: out of host memory", who);
  s->width = width, s->height = height, s->patch = o.patch, s->max_patches = o.max_patches;
  s->pixels = (uint32_t)width * (uint32_t)height;
  const uint32_t blocks = (s->pixels + BLOCK - 1) / BLOCK;
  s->nparts = blocks < (uint32_t)MAX_PARTS ? blocks : (uint32_t)MAX_PARTS;
  s->chunks = ((uint32_t)o.patch * (uint32_t)o.patch + SCORE_PIXELS - 1) / SCORE_PIXELS;
  hipError_t e = hipMalloc((void**)&s->d_part, part_bytes(s));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_corners, corner_bytes(s));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_partials, partial_bytes(s));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_records, record_bytes(s));
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_corners, RING * corner_bytes(s), hipHostMallocDefault);
  for (int k = 0; k < RING; k++)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->slot_done[k], hipEventDisableTiming);
  if ((rc = pt_stage::create_events(who, e, s, pt_patches_destroy)) != PT_OK) return rc;
  *out = s;
  return PT_OK;
}

int pt_patches_workspace_bytes(const pt_patches* s, uint64_t* bytes) {
  if (!s || !bytes) return pt_fail(PT_EINVAL, "pt_patches_workspace_bytes: null %s", s ? "output pointer" : "session");
  *bytes = part_bytes(s) + corner_bytes(s) + partial_bytes(s) + record_bytes(s);
  return PT_OK;
}

int pt_patches_prepare(pt_patches* s, const float* d_train, void* hip_stream) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_prepare: null session");
  if (!d_train) return pt_fail(PT_EINVAL, "pt_patches_prepare: null d_train");
  return enqueue_prepare(s, d_train, (hipStream_t)hip_stream);
}

int pt_patches_run_prepare(pt_patches* s, const float* d_train, float* ms_out) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_run_prepare: null session");
  if (!d_train) return pt_fail(PT_EINVAL, "pt_patches_run_prepare: null d_train");
  return pt_stage::run_timed(s->ev0, s->ev1, ms_out, [&] { return enqueue_prepare(s, d_train, nullptr); });
}

int pt_patches_score(pt_patches* s, const float* d_train, int n, const int32_t* corners, void* hip_stream) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_score: null session");
  const int rc = check_corners("pt_patches_score", s, d_train, n, corners);
  if (rc != PT_OK) return rc;
  return enqueue_score(s, d_train, n, corners, (hipStream_t)hip_stream);
}

int pt_patches_run_score(pt_patches* s, const float* d_train, int n, const int32_t* corners, float* ms_out) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_run_score: null session");
  const int rc = check_corners("pt_patches_run_score", s, d_train, n, corners);
  if (rc != PT_OK) return rc;
  return pt_stage::run_timed(s->ev0, s->ev1, ms_out, [&] { return enqueue_score(s, d_train, n, corners, nullptr); });
}

int pt_patches_gather(pt_patches* s, const float* d_train, const float* d_gt, int gt_pixel_stride, int n, const int32_t* corners,
                      float* d_inputs, float* d_targets, void* hip_stream) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_gather: null session");
  const GatherCall a{d_train, d_gt, gt_pixel_stride, n, corners, d_inputs, d_targets};
  const int rc = check_gather("pt_patches_gather", s, a);
  if (rc != PT_OK) return rc;
  return enqueue_gather(s, a, (hipStream_t)hip_stream);
}

int pt_patches_run_gather(pt_patches* s, const float* d_train, const float* d_gt, int gt_pixel_stride, int n, const int32_t* corners,
                          float* d_inputs, float* d_targets, float* ms_out) {
  if (!s) return pt_fail(PT_EINVAL, "pt_patches_run_gather: null session");
  const GatherCall a{d_train, d_gt, gt_pixel_stride, n, corners, d_inputs, d_targets};
  const int rc = check_gather("pt_patches_run_gather", s, a);
  if (rc != PT_OK) return rc;
  return pt_stage::run_timed(s->ev0, s->ev1, ms_out, [&] { return enqueue_gather(s, a, nullptr); });
}

int pt_patches_result(pt_patches* s, int patch_index, pt_patches_values* out) {
  if (!s || !out) return pt_fail(PT_EINVAL, "pt_patches_result: null %s", s ? "output pointer" : "session");
  if (patch_index < 0 || patch_index >= s->last_patches)
    return pt_fail(PT_EINVAL, "pt_patches_result: patch_index %d outside the last score call's %d patches", patch_index, s->last_patches);
  Sums r;
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(&r, s->d_records + patch_index, sizeof(Sums), hipMemcpyDeviceToHost));
  out->colour_s1 = (int64_t)r.v[0], out->colour_a = r.v[1], out->colour_b = r.v[2], out->colour_c = r.v[3];
  out->normal_s1 = (int64_t)r.v[4], out->normal_a = r.v[5], out->normal_b = r.v[6], out->normal_c = r.v[7];
  out->values = 3ull * (uint64_t)s->patch * (uint64_t)s->patch;
  out->var_colour = variance(r.v, out->values);
  out->var_normal = variance(r.v + 4, out->values);
  out->score = out->var_colour + out->var_normal;
  return PT_OK;
}

}  // extern "C"
