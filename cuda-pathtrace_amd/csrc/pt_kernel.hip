// pt_kernel.hip -- the per-pixel Monte-Carlo megakernel for gfx950 (MI355X).
//
// Replaces src/pathtrace.cu's pixel_kernel (:203-257) and setup_random (:259-266).
// One lane = one pixel, lanes of a wave64 are 64 CONSECUTIVE COLUMNS of one image row
// (the reference maps adjacent threads to adjacent rows, i.e. a 56*W-byte lane stride).
// The sphere list is staged once per workgroup into LDS; generator state, ray, throughput,
// AOV sums and the four Welford accumulators live in VGPRs for the whole frame.
#include "pt_trace.h"

#pragma clang fp contract(off)

// The kernel variants, one row each (VariantInfo, pt_kernel.h; what the variants are: the list there).  A new variant or a new
// build flavour is registered HERE: the kernels below, the selector, the launchers and pt_capi.hip follow the row.
static constexpr int kNumVariants = 15;
static constexpr int kT = PT_BLOCK_THREADS, kTG = PT_GRID_BLOCK_THREADS, kTW = PT_GRID_WIDE_THREADS;
static constexpr int kW = PT_MIN_WAVES, kWG = PT_GRID_MIN_WAVES, kWD = PT_GRID12_MIN_WAVES, kWP = PT_POOL_MIN_WAVES;
static constexpr VariantInfo kVariants[kNumVariants] = {
    //        product lanes threads lean        LDS extra      grid            wide   ref    resume frames chunk family       chunks waves loop               tracer kernel
    /*  0 */ {true,  1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   0,     0},
    // 1-5, 7: measured negative results and stepping stones
    /*  1 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   1,     1},
    /*  2 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   2,     2},
    /*  3 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PACKED, PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   3,     3},
    /*  4 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   4,     4},
    /*  5 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_SAMPLES,   5,     5},
    /*  6 */ {true,  1, kT,  PT_LEAN_BIG,    PT_LDS_WALLS,  PT_GRID_NONE,   false, true,  true,  true,  PT_CHUNK_ONE_LANE, true,  kW,   PT_LOOP_SAMPLES,   6,     6},
    /*  7 */ {false, 1, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, false, false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_PAIRS,     6,     7},
    /*  8 */ {true,  4, kT,  PT_LEAN_BIG,    PT_LDS_PLAIN,  PT_GRID_NONE,   false, true,  false, false, PT_CHUNK_SPLIT,    true,  0,    PT_LOOP_SAMPLES,   6,     8},
    /*  9 */ {true,  2, kT,  PT_LEAN_NEVER,  PT_LDS_PLAIN,  PT_GRID_NONE,   false, true,  false, false, PT_CHUNK_SPLIT,    true,  0,    PT_LOOP_SAMPLES,   6,     9},
    /* 10 */ {true,  1, kT,  PT_LEAN_BIG,    PT_LDS_PLAIN,  PT_GRID_NONE,   false, false, true,  false, PT_CHUNK_NONE,     false, kW,   PT_LOOP_REGEN,     6,     10},
    // 11 (the grid walk with every lane testing its own spheres) and 12: superseded by 13, kept for A/B
    /* 11 */ {false, 1, kTG, PT_LEAN_ALWAYS, PT_LDS_PLAIN,  PT_GRID_LANE,   false, false, false, false, PT_CHUNK_NONE,     false, kWG,  PT_LOOP_REGEN,     11,    11},
    /* 12 */ {false, 1, kTG, PT_LEAN_ALWAYS, PT_LDS_PLAIN,  PT_GRID_LANE,   false, false, false, false, PT_CHUNK_NONE,     false, kWD,  PT_LOOP_DECOUPLED, 11,    12},
    /* 13 */ {true,  1, kTG, PT_LEAN_ALWAYS, PT_LDS_PLAIN,  PT_GRID_POOLED, false, false, true,  false, PT_CHUNK_GRID,     true,  kWP,  PT_LOOP_REGEN,     13,    13},
    // 14 is variant 13's kernel with WIDE (there is no VAR = 14 build).  It cannot chunk: the host has never chunked it, although
    // that kernel could and its sample cap is the grid family's
    /* 14 */ {true,  1, kTW, PT_LEAN_ALWAYS, PT_LDS_PLAIN,  PT_GRID_POOLED, true,  false, true,  false, PT_CHUNK_GRID,     false, kWP,  PT_LOOP_REGEN,     13,    13},
};
static constexpr VariantInfo kNoVariant = {false, 1, kT, PT_LEAN_NEVER, PT_LDS_PLAIN, PT_GRID_NONE, false, false, false, false, PT_CHUNK_NONE, false, kW, PT_LOOP_SAMPLES, 0, 0};

// What the kernels below rely on, so that a row and the builds behind it cannot disagree (r: a row, k: the row of the kernel that
// executes it; inside pixel_kernel / pixel_kernel_split the other half: a build exists only where its kernel's row announces it)
template <class P>
constexpr bool every_row(P holds) {
  for (int i = 0; i < kNumVariants; i++)
    if (!holds(i, kVariants[i], kVariants[kVariants[i].kernel])) return false;
  return true;
}
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo&) { return r.kernel >= 0 && r.kernel < kNumVariants; }), "every row's kernel is a row");
static_assert(every_row([](int i, const VariantInfo& r, const VariantInfo& k) { return (r.wide || r.kernel == i) && !k.wide; }), "only a wide row runs another row's kernel");
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo& k) { return !r.wide || (k.grid == PT_GRID_POOLED && r.threads == kTW); }), "a wide row names a pooled-grid kernel");
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo& k) { return (!r.resume || k.resume) && (!r.frames || k.frames) && (!r.ref_builds || k.ref_builds); }),
              "a row's resume, frames and reference-configuration builds are its kernel's");
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo& k) {
                return r.lean == k.lean && r.lds_extra == k.lds_extra && r.grid == k.grid && r.min_waves == k.min_waves && r.loop == k.loop && r.tracer == k.tracer;
              }), "a wide row differs from its kernel's in the workgroup only");
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo&) { return !r.frames || (r.lanes == 1 && r.ref_builds); }), "frames builds: one-lane rows, reference configurations");
static_assert(every_row([](int, const VariantInfo& r, const VariantInfo&) { return !r.split() || (!r.resume && !r.wide && r.grid == PT_GRID_NONE); }), "pixel_kernel_split: no resume, wide or grid builds");
// the rows a kernel's template arguments name: pixel_kernel_split's by its lanes per pixel, a WIDE build's launch by its kernel
constexpr int split_row(int lanes) {
  for (int i = 0; i < kNumVariants; i++)
    if (kVariants[i].split() && kVariants[i].lanes == lanes) return i;
  return -1;
}
constexpr int launch_row(int kernel, bool wide) {
  for (int i = 0; wide && i < kNumVariants; i++)
    if (kVariants[i].wide && kVariants[i].kernel == kernel) return i;
  return wide ? -1 : kernel;
}

namespace pt {

// pixel_kernel: src/pathtrace.cu:203-257
// LEAN selects the geometry-only LDS layout of many-sphere scenes (pt_scene_lds.h) at compile time, so the
// 9-sphere kernels carry no trace of it.
// REFB != 0 builds the kernel for the reference's own scene size -- 9 spheres (Scene.h:23) -- and a fixed bounce cap as
// compile-time constants: REFB = 5 is the reference's MAX_BOUNCES (pathtrace.cu:7), REFB = 8 the interactive configuration
// (BASELINE.json configs[4]).  No generic loops, no index-width arithmetic, and a hot loop that is a third smaller.
// (VAR is a row of kVariants: the kernel reads what it is from that row; WIDE only launches it as the wide row that names it)
template <int VAR, bool WIDE = false>
constexpr int kBlockThreads = kVariants[launch_row(VAR, WIDE)].threads;

// the reference-configuration builds of variant 6 with the XORWOW generator fit 96 registers (12 bytes of spills, in cold code:
// WRITE_SIZE stays at the algorithmic bytes): five waves per SIMD instead of four (headline frame 50.12 -> 49.81 ms, three
// alternating runs each, profiles/r03/README.md).  The philox builds spilled warm then (WRITE_SIZE 143 -> 400 MB per frame) and
// gained nothing; after the bit-operation work of round 3 the 5-bounce build fits 96 registers with ONE spilled word (a reload
// per sample) and gains 1.5 % (48.73 -> 47.98 ms, profiles/r03/README.md); the 8-bounce build (4 words) does not (0.0963 -> 0.0971 ms)
// and keeps four waves, like every other build.
template <int VAR, int REFB, int RNG>
constexpr int kMinWavesR = (kVariants[VAR].ref_builds && REFB != 0) ? (RNG == PT_RNG_XORWOW ? PT_REF_MIN_WAVES : (REFB == 5 ? PT_REF_MIN_WAVES_PHILOX : kVariants[VAR].min_waves))
                                                                      : kVariants[VAR].min_waves;

// ---- the hand-over chain of sample chunking (what it is for: pixel_kernel below) ------------------------------------------
// chunk_flag[block]: bits 0-30 = chunks of the pixel block that have completed, bit 31 (PT_CHUNK_FAILED) = the chain is broken.
// Wait for the predecessor of chunk `chunk`.  The wait is bounded in TIME (s_memrealtime) and giving up is an ERROR the host
// sees (device error word -> PT_EKERNEL or a repair launch, pt_capi.hip), never a silent frame.  A workgroup that gives up, or
// finds the chain already broken, marks the chain broken and leaves WITHOUT touching the frame, the hand-over buffer or the
// generator state -- so do all its successors (they can only ever see the mark: the count stops below them), the last chunk
// included, and the last chunk is the only one that writes the frame and the generator state.  Hence after a launch every
// pixel block is either complete (count == chunks: frame and state exactly the reference's) or untouched (frame and state as
// before the launch), which is what lets the host render the untouched blocks again, unchunked (a.repair).
// Returns true (workgroup-uniform) when the caller has to leave.
__device__ __forceinline__ bool chunk_wait(const PixelKernelArgs& a, uint32_t block_id, uint32_t chunk) {
  __shared__ uint32_t s_pred;
  if (threadIdx.x == 0) {
    const uint64_t t0 = wall_clock64();
    uint32_t spins = 0, f;
    for (;;) {
      f = __hip_atomic_load(a.chunk_flag + block_id, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      if ((f & PT_CHUNK_FAILED) != 0u || f >= chunk) break;
      __builtin_amdgcn_s_sleep(32);
      if ((++spins & 255u) == 0u && wall_clock64() - t0 > a.chunk_wait_ticks) {
        f = PT_CHUNK_FAILED;
        break;
      }
    }
    if ((f & PT_CHUNK_FAILED) != 0u) {
      if (a.err_word) atomicOr(a.err_word, PT_DEVERR_CHUNK_CHAIN);
      __hip_atomic_fetch_or(a.chunk_flag + block_id, PT_CHUNK_FAILED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_pred = f;
  }
  __syncthreads();
  return (s_pred & PT_CHUNK_FAILED) != 0u;
}

// chunk `chunk` of the block is complete: everything it stored is visible device-wide before the count says so.  The count
// only grows and never clears the failure mark (a predecessor that was merely slow may finish after its successor gave up).
__device__ __forceinline__ void chunk_publish(const PixelKernelArgs& a, uint32_t block_id, uint32_t chunk) {
  __syncthreads();  // every wave's stores are issued ...
  if (threadIdx.x == 0) {
    __threadfence();  // ... and visible device-wide before the flag says so
#if PT_BUILD_EXPERIMENTS  // lab library: a deliberately broken chain for the failure-path tests
    if ((a.debug & PT_DEBUG_DROP_CHUNK_FLAG) && block_id == 0u && chunk == 0u) return;
#endif
    __hip_atomic_fetch_max(a.chunk_flag + block_id, chunk + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// FRAMES (round 5, pt_launch_frames_kernel below): the launch renders a BATCH of frames with known cameras (which travel as
// kernel arguments too), each into its own buffer, starting from zeroed sums.  Per pixel the operations and their order are those
// of fr_count single-frame launches.  What links two frames is the generator (the reference's d_states carries every pixel's
// XORWOW state from one Render() to the next: pathtrace.cu:212,256), hence two shapes:
//  * XORWOW: a workgroup keeps its pixel block for the whole batch and LOOPS over the frames; the generator simply stays in
//    its registers.  What goes is the ramp and tail of fr_count launches, the per-launch staging and the state traffic.  (First
//    built as one workgroup per (frame, block) with the state handed on through the sample chunks' flags: a workgroup that
//    becomes resident while its predecessor still runs only waits, and the dispatcher cannot pass it over for one that is
//    ready -- 0.1145 ms per frame against 0.097 as single launches; profiles/r05/cfg5_frames.txt.  Also measured, no effect:
//    scattering the pixel blocks over the workgroups, so that no CU holds four neighbouring blocks -- 0.0936 vs 0.0938.)
//  * the counter-based generator is re-keyed per frame, so its frames are independent: one workgroup per (frame, pixel block),
//    frame-major -- the next frame's workgroups fill the slots the current one's leave (and the fifth slot per CU a single
//    1024-workgroup frame cannot use).
//
// RESUME (progressive passes, pt_capi.hip): the launch renders samples [sample_begin, spp) of an spp-sample frame.  It starts
// from the session's record -- the state a chunk hands to the next one, same words, same [word][pixel] layout -- unless
// sample_begin is 0, and ends by writing BOTH the frame of all spp samples and the record.  Per pixel, a session performs the
// operations of one spp-sample launch in their order (EXACTNESS.md A.19); the one difference is that a session always jitters.
//
// ADAPTIVE (RESUME builds only; adaptive progressive passes, pt_adaptive.hip): lane slot -> pixel list[slot] of the session's
// active list (raster order, *list_len entries, written on the device by the selection just before).  Slots past the length
// are inactive lanes; a workgroup whose first slot lies past it leaves before staging anything.  The pass writes only the
// record: the frame is formed afterwards for every pixel at its own count (pt_launch_adaptive_finalize).
template <bool FRAMES, bool RESUME = false, bool ADAPTIVE = false> struct KernelArgsOf { typedef PixelKernelArgs type; };
template <> struct KernelArgsOf<true, false, false> { typedef FramesKernelArgs type; };  // (the cameras travel as kernel arguments too)
template <> struct KernelArgsOf<false, true, false> { typedef ResumeKernelArgs type; };
template <> struct KernelArgsOf<false, true, true> { typedef AdaptiveKernelArgs type; };
template <bool FRAMES, bool RESUME, bool ADAPTIVE> __device__ __forceinline__ PixelKernelArgs& base_args(typename KernelArgsOf<FRAMES, RESUME, ADAPTIVE>::type& args) {
  if constexpr (FRAMES || RESUME) return args.base; else return args;
}

// WIDE (variant 13 only; the launcher's "variant 14"): 1024-thread workgroups, one per CU -- pt_grid.h, grid_max_entries
// (the 8-bounce XORWOW resume build: at five waves it spills two words its twin does not -- four waves, like the batch build)
template <int RNG, int VAR, bool LEAN = false, int REFB = 0, bool FRAMES = false, bool WIDE = false, bool RESUME = false, bool ADAPTIVE = false>
__global__ void __launch_bounds__((kBlockThreads<VAR, WIDE>), (((FRAMES || (RESUME && REFB == 8)) && RNG == PT_RNG_XORWOW) ? PT_MIN_WAVES : kMinWavesR<VAR, REFB, RNG>)) PT_KERNEL_ATTR
pixel_kernel(typename KernelArgsOf<FRAMES, RESUME, ADAPTIVE>::type args) {  // (an XORWOW batch has one workgroup per pixel block for all its frames: the
                                                           // interactive shape fills four of a CU's five slots, so that build takes 128 registers)
  PixelKernelArgs& a = base_args<FRAMES, RESUME, ADAPTIVE>(args);
  constexpr VariantInfo K = kVariants[VAR];  // this kernel's row
  constexpr bool POOLED = K.grid == PT_GRID_POOLED;
  static_assert(K.kernel == VAR && !K.split() && kVariants[launch_row(VAR, WIDE)].wide == WIDE, "a pixel_kernel build is a one-lane row's own kernel, WIDE a wide row's");
  static_assert(!ADAPTIVE || RESUME, "adaptive passes are resume builds");
  uint32_t n_active = 0u;  // (adaptive: the length of the active list; workgroup-uniform)
  if constexpr (ADAPTIVE) {
    n_active = __builtin_amdgcn_readfirstlane(*args.list_len);
    if (blockIdx.x * (uint32_t)kBlockThreads<VAR, WIDE> >= n_active) return;  // no active slot in this workgroup
  }
  // a batch of frames, two shapes (head of this section): the counter-based generator's frames are independent -- one workgroup
  // per (frame, pixel block), frame-major; XORWOW's are a chain per pixel -- one workgroup per pixel block, looping over the frames
  constexpr bool FRAME_GRID = FRAMES && RNG == PT_RNG_PHILOX, FRAME_LOOP = FRAMES && !FRAME_GRID;
  uint32_t fr = 0u, fr_count = 1u, first_block = blockIdx.x;
  auto load_camera = [&](uint32_t f) {
    if constexpr (FRAMES) {
      // by scalar loads from the argument segment itself (indexing the by-value struct with a run-time index would make the
      // compiler copy all of it to scratch memory)
      typedef const __attribute__((address_space(4))) float* cfloats;
      typedef const __attribute__((address_space(4))) char* cbytes;
      const cfloats cam = (cfloats)((cbytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FramesKernelArgs, cams)) + 15u * f;
#pragma unroll
      for (int k = 0; k < 12; k++) a.basis[k] = cam[k];
#pragma unroll
      for (int k = 0; k < 3; k++) a.eye[k] = cam[12 + k];
    }
  };
  if constexpr (FRAMES) fr_count = args.frames;
  if constexpr (FRAME_GRID) {
    const uint32_t n_blocks = (a.tile_pixels + kBlockThreads<VAR, WIDE> - 1) / kBlockThreads<VAR, WIDE>;
    fr = blockIdx.x / n_blocks;  // (workgroup-uniform)
    first_block = blockIdx.x - fr * n_blocks;
    load_camera(fr);  // before the scene image is staged for this frame's eye
  }
  constexpr bool REF = REFB != 0;
  constexpr bool CHUNKS = K.chunk_build(REF) && !FRAMES && !RESUME;
  static_assert(!REF || K.ref_builds, "reference-configuration builds: the rows that announce them");
  static_assert(!LEAN ? K.lean != PT_LEAN_ALWAYS : K.lean != PT_LEAN_NEVER, "the LDS layouts of the row");
  static_assert(!FRAMES || (K.frames && REF), "frame batches: reference-configuration builds of the rows with frames (variant 6)");
  static_assert(!RESUME || (!FRAMES && K.resume), "progressive passes: the rows with resume (variants 6, 10, 13; 14 = WIDE)");
  int sample_begin = 0;  // (a pass: the samples the session already holds; a.spp is the session's count after the pass)
  if constexpr (RESUME) sample_begin = args.sample_begin;
  const int pass_spp = a.spp - sample_begin;  // the cost heuristics below look at what this launch renders
  if constexpr (REF) {
    a.n_spheres = 9;
    a.max_bounces = REFB;
  }
  if constexpr (CHUNKS) {
    // repair launch (pt_capi.hip, after a chunked launch whose chain broke): unchunked, and only for the pixel blocks that
    // launch left untouched -- the ones it completed are not rendered a second time
    if (a.repair != 0u && __hip_atomic_load(a.chunk_flag + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.repair) return;
  }
  extern __shared__ float4 lds_scene[];
  SceneLds sc = stage_scene<K.lds_extra == PT_LDS_PACKED>(a.spheres, a.n_spheres, lds_scene, LEAN, mk3(a.eye[0], a.eye[1], a.eye[2]), a.spp);
  // variants with a lean build run their LDS build only on scenes up to PT_SCREEN_MAX_SPHERES (launcher): the
  // many-sphere path is not even compiled into it, which keeps the hot loop's code small
  sc.small_only = !LEAN && K.lean == PT_LEAN_BIG;
  // the 5-bounce reference-configuration builds of variant 6 screen secondary rays against the faced wall of each axis only
  // (pt_walls.h; the 8-bounce interactive build keeps the nine-sphere screen: DESIGN.md section 8)
  constexpr bool kWalls = K.lds_extra == PT_LDS_WALLS && REFB == 5 && !LEAN;
  if constexpr (kWalls) stage_walls(sc, a.spheres, a.n_spheres);
  constexpr bool kRegen = K.loop == PT_LOOP_REGEN, kDecoupled = K.loop == PT_LOOP_DECOUPLED;
  GridLds grid;
  if constexpr (K.grid != PT_GRID_NONE) {  // the frame's grid, built by build_grid_kernel just before this launch
    grid = stage_grid<POOLED>(a.spheres, a.n_spheres, a.accel, lds_scene + a.scene_lds_f4);  // after the two small tables
    sc.grid = &grid;
    if constexpr (POOLED)  // the test pool of each wave follows the grid image (16-byte aligned)
      sc.pool = reinterpret_cast<char*>(lds_scene + a.scene_lds_f4) + ((grid_lds_bytes(a.n_spheres, true, kBlockThreads<VAR, WIDE>) + 15) & ~(size_t)15);
  }

  // Sample chunking (REF builds of variant 6, variant 13): workgroup blockIdx.x = chunk * n_blocks + block renders samples
  // [chunk * per, (chunk + 1) * per) of its 256 pixels and hands generator, sums and Welford accumulators to the next chunk
  // through chunk_state.  Forward progress (DESIGN.md section 3 ("sample chunking")): every dispatcher hands out its workgroups in
  // increasing index order, so by induction on the lowest unfinished index the predecessor of a waiting workgroup is resident
  // or done -- and the lowest unfinished one never waits.  That is a property of today's hardware, not of the programming
  // model, so the wait is bounded in time and giving up raises the renderer's error word (PT_EKERNEL), never a silent frame.
  // Same operations per pixel in the same order; what changes is that a frame of few, long workgroups becomes one of many
  // short ones (tools/shape_sweep.py: why).
  uint32_t block_id = FRAMES ? first_block : blockIdx.x, chunk = 0u, n_chunks = 1u;
  if constexpr (CHUNKS) {
    if (a.chunks > 1u) {
      const uint32_t n_blocks = (a.tile_pixels + kBlockThreads<VAR, WIDE> - 1) / kBlockThreads<VAR, WIDE>;
      n_chunks = a.chunks;
      chunk = blockIdx.x / n_blocks;
      block_id = blockIdx.x - chunk * n_blocks;
    }
  }
  const uint32_t slot = block_id * kBlockThreads<VAR, WIDE> + threadIdx.x;
  const bool active = ADAPTIVE ? slot < n_active : slot < a.tile_pixels;  // lanes past the tile (the list) stay for the cooperative parts
  const uint32_t tp = [&]() -> uint32_t {  // pixel index inside the tile
    if constexpr (ADAPTIVE) return active ? args.list[slot] : 0u; else return slot;
  }();
  const int row = a.row_begin + (int)(tp / (uint32_t)a.width);
  const int col = (int)(tp % (uint32_t)a.width);
  const uint32_t id = (uint32_t)row * (uint32_t)a.width + (uint32_t)col;  // :206

  Rng<RNG> rng;
  if constexpr (RNG == PT_RNG_XORWOW) {
    if (a.rng_state && active) {  // :212
      const uint32_t* s = a.rng_state + (size_t)tp * 6;
      rng.st = Xorwow{s[0], s[1], s[2], s[3], s[4], s[5]};
    } else {
      xorwow_init(rng.st, (uint64_t)id + a.seed);  // :265
    }
  } else {
    rng.k0 = (uint32_t)a.seed;
    rng.k1 = (uint32_t)(a.seed >> 32) ^ a.frame;
    rng.pix = id;
  }

  const bool pow2_image = ((a.width & (a.width - 1)) == 0) && ((a.height & (a.height - 1)) == 0);  // wave-uniform
  const float inv_w = 1.0f / (float)a.width, inv_h = 1.0f / (float)a.height;  // exact for powers of two

  // (the frame loop of a batch is a backward goto that exists in the FRAME_LOOP builds only: every other build's code is,
  // instruction for instruction, what it was without it -- a `for` with one trip was not, and the headline kernel's allocation is touchy)
frame_top:
  if constexpr (FRAME_LOOP) {
    load_camera(fr);
    if (fr > 0u) {  // the scene image's eye part (SceneLds::eyeg: off and c of :73,76 for rays from THIS frame's eye), as stage_scene forms it
      __syncthreads();  // every wave has finished the previous frame's primary rays
      for (int i = threadIdx.x; i < a.n_spheres; i += blockDim.x) {
        const float4 g = sc.geom[i];
        const F3 off = mk3(a.eye[0] - g.x, a.eye[1] - g.y, a.eye[2] - g.z);
        sc.eyeg[i] = make_float4(off.x, off.y, off.z, dot(off, off) - g.w);
      }
      __syncthreads();
    }
  }
  if constexpr (FRAMES && RNG == PT_RNG_PHILOX) rng.k1 = (uint32_t)(a.seed >> 32) ^ (a.frame + fr);
  const F3 B0 = mk3(a.basis[0], a.basis[1], a.basis[2]), B1 = mk3(a.basis[3], a.basis[4], a.basis[5]);
  const F3 B2 = mk3(a.basis[6], a.basis[7], a.basis[8]), B3 = mk3(a.basis[9], a.basis[10], a.basis[11]);
  const F3 eye = mk3(a.eye[0], a.eye[1], a.eye[2]);

  Welford var[4] = {{0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}};
  TraceOutput L{mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0), 0.0f};
  int i_begin = sample_begin, i_end = a.spp;
  if constexpr (RESUME) {
    if (sample_begin > 0 && active) {  // the session's record (written by the pass before: no other launch touches it)
      const uint32_t* rec = args.session;
      auto ld = [&](int w) { return rec[(size_t)w * a.tile_pixels + tp]; };
      auto ldf = [&](int w) { return __uint_as_float(ld(w)); };
      L.color = mk3(ldf(PT_REC_COLOR), ldf(PT_REC_COLOR + 1), ldf(PT_REC_COLOR + 2));
      L.normal = mk3(ldf(PT_REC_NORMAL), ldf(PT_REC_NORMAL + 1), ldf(PT_REC_NORMAL + 2));
      L.albedo = mk3(ldf(PT_REC_ALBEDO), ldf(PT_REC_ALBEDO + 1), ldf(PT_REC_ALBEDO + 2));
      L.depth = ldf(PT_REC_DEPTH);
      const int n0 = (int)ld(PT_REC_N_COLOR), n1 = (int)ld(PT_REC_N_HIT);
#pragma unroll
      for (int k = 0; k < 4; k++) var[k] = Welford{k == 0 ? n0 : n1, ldf(PT_REC_MEAN + 2 * k), ldf(PT_REC_M2 + 2 * k)};
      if constexpr (RNG == PT_RNG_XORWOW) rng.st = Xorwow{ld(PT_REC_RNG), ld(PT_REC_RNG + 1), ld(PT_REC_RNG + 2), ld(PT_REC_RNG + 3), ld(PT_REC_RNG + 4), ld(PT_REC_RNG + 5)};
    }
  }
  if constexpr (CHUNKS) {
    if (n_chunks > 1u) {
      const int per = (a.spp + (int)n_chunks - 1) / (int)n_chunks;
      i_begin = (int)chunk * per;
      i_end = i_begin + per < a.spp ? i_begin + per : a.spp;
      if (chunk > 0u) {
        if (chunk_wait(a, block_id, chunk)) return;  // the chain of this pixel block is broken: nothing of the block is written
        if (active) {
          auto ld = [&](int w) { return __hip_atomic_load(a.chunk_state + (size_t)w * a.tile_pixels + tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
          auto ldf = [&](int w) { return __uint_as_float(ld(w)); };
          L.color = mk3(ldf(PT_REC_COLOR), ldf(PT_REC_COLOR + 1), ldf(PT_REC_COLOR + 2));
          L.normal = mk3(ldf(PT_REC_NORMAL), ldf(PT_REC_NORMAL + 1), ldf(PT_REC_NORMAL + 2));
          L.albedo = mk3(ldf(PT_REC_ALBEDO), ldf(PT_REC_ALBEDO + 1), ldf(PT_REC_ALBEDO + 2));
          L.depth = ldf(PT_REC_DEPTH);
          const int n0 = (int)ld(PT_REC_N_COLOR), n1 = (int)ld(PT_REC_N_HIT);  // the three first-hit accumulators count together (welford_update3)
#pragma unroll
          for (int k = 0; k < 4; k++) var[k] = Welford{k == 0 ? n0 : n1, ldf(PT_REC_MEAN + 2 * k), ldf(PT_REC_M2 + 2 * k)};
          if constexpr (RNG == PT_RNG_XORWOW) rng.st = Xorwow{ld(PT_REC_RNG), ld(PT_REC_RNG + 1), ld(PT_REC_RNG + 2), ld(PT_REC_RNG + 3), ld(PT_REC_RNG + 4), ld(PT_REC_RNG + 5)};
        }
      }
    }
  }

  auto primary_ray = [&](Rng<RNG>& g, F3& dir) {  // :221-229
    float sx = (float)row, sy = (float)col;
    if (RESUME || a.spp != 1) {  // (a session cannot know its final count: it always jitters)
      float jx, jy;
      g.jitter(jx, jy);
      sx += jx * 1.0f - 0.5f;
      sy += jy * 1.0f - 0.5f;
    }
    if (pow2_image) {  // x / 2^k == x * 2^-k exactly: spares two correctly rounded divisions per sample
      sx *= inv_h;
      sy *= inv_w;
    } else {
      sx /= (float)a.height;  // contract C7
      sy /= (float)a.width;
    }
    dir = lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx);
  };

  // the primary direction for screen position (sx, sy) in pixel units, by primary_ray's own formula (footprint analyses)
  auto dir_at = [&](float sx, float sy) {
    if (pow2_image) {
      sx *= inv_h;
      sy *= inv_w;
    } else {
      sx /= (float)a.height;
      sy /= (float)a.width;
    }
    return lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx);
  };
  if constexpr (REF) {
#ifndef PT_NO_FOOTPRINT
    // once per pixel: the spheres this pixel's primary rays can return; the wave ranks the union at bounce 0
    if (pass_spp >= PT_FOOTPRINT_MIN_SPP) {
      const uint32_t mine = active ? primary_candidates(sc, a.n_spheres, (float)row, (float)col, dir_at) : 0u;
      uint32_t wave_mask = 0u;
#pragma unroll
      for (int j = 0; j < 9; j++) wave_mask |= (__builtin_amdgcn_ballot_w64(((mine >> j) & 1u) != 0u) != 0ull) ? (1u << j) : 0u;
      sc.prim_mask = wave_mask;
    }
#endif
  }

  int i = active ? i_begin : i_end;  // inactive lanes trace nothing ([i_begin, i_end): all samples unless the frame is chunked)
  bool prim_ok = false;  // variant 13: this pixel's primary rays take their spheres from the pixel's list instead of walking the grid
  if constexpr (POOLED && PT_PRIMLIST) {
    // once per pixel and workgroup: the grid spheres the pixel's primary rays can return (pt_primlist.h)
    if (grid.valid && pass_spp >= PT_PRIMLIST_MIN_SPP && a.max_bounces >= 1) {
      int k = 0;
      const uint32_t slot = grid.h.prim_base + (uint32_t)kPrimEntriesPerLane * threadIdx.x;
      prim_ok = build_primary_list(grid, a.spheres, a.n_spheres, eye, (float)row, (float)col, active, dir_at, pool_of_wave(sc.pool).ring,
                                   const_cast<uint2*>(grid.cells), slot, k);
      // a pixel that sees nothing at all: every sample is `output.color += color; return` (:157-161) after its jitter draws
      if (prim_ok & (k == 0) & ((grid.h.n_big & 0xFFFFu) == 0u)) {
        for (; i < i_end; i++) {
          if constexpr (RNG == PT_RNG_XORWOW) {  // (philox: begin_sample only positions the counter)
            if (RESUME || a.spp != 1) {
              float jx, jy;
              rng.jitter(jx, jy);  // :223-224
            }
          }
          L.color = L.color + mk3(0.0f, 0.0f, 0.0f);  // :159
        }
      }
    }
  }
  if constexpr (kRegen) {
    // Path regeneration (the bit-exact form of active-ray compaction for a kernel whose accumulators are
    // per lane): the sample loop and the bounce loop are flattened into one per-lane state machine, so a
    // lane whose path left the scene starts its next sample at once instead of idling until the longest
    // path of the wave has finished its bounces.  Every lane still executes exactly the reference's
    // sequence for its pixel (same draws, same sums, same Welford updates, same order); only the
    // alignment BETWEEN lanes changes.  Pays in open scenes, costs the unrolled path in closed ones.
    int n = 0;  // depth of the current path; 0 = start a new sample
    F3 o = eye, d = eye;
    F3 color = mk3(0.0f, 0.0f, 0.0f), mask = mk3(1.0f, 1.0f, 1.0f);
    // issue priority by progress, as in the one-lane loop below (there: why); the progress of a wave is that of its first lane
    const int span = i_end - i_begin;  // this workgroup's samples
    const bool by_progress = span >= PT_PRIO_MIN_SPP_REGEN;
    const int q1 = i_begin + span / 4, q2 = i_begin + span / 2, q3 = i_end - span / 4;
    int last_band = -1;
    // (variant 13: the wave stays together until its LAST lane is done -- lanes that have finished their samples keep going through
    // the nearest-hit search as helpers of the pooled sphere tests, which otherwise run ever emptier towards the end of every workgroup)
    for (;;) {
      const bool live = i < i_end;
      if constexpr (POOLED && PT_POOL_HELPERS) {
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;
      } else {
        if (!live) break;
      }
      if (by_progress) {
        int iu;  // the first lane that still works
        if constexpr (POOLED && PT_POOL_HELPERS) iu = __builtin_amdgcn_readlane(i, __builtin_ctzll(__builtin_amdgcn_ballot_w64(live)));
        else iu = __builtin_amdgcn_readfirstlane(i);
        const int band = (iu >= q1 ? 1 : 0) + (iu >= q2 ? 1 : 0) + (iu >= q3 ? 1 : 0);
        if (band != last_band) {  // wave-uniform
          last_band = band;
          if (band == 0) __builtin_amdgcn_s_setprio(3);
          else if (band == 1) __builtin_amdgcn_s_setprio(2);
          else if (band == 2) __builtin_amdgcn_s_setprio(1);
          else __builtin_amdgcn_s_setprio(0);
        }
      }
      if (live & (n == 0)) {  // :219-229
        rng.begin_sample((uint32_t)i);
        primary_ray(rng, d);
        o = eye;
        color = mk3(0.0f, 0.0f, 0.0f);
        mask = mk3(1.0f, 1.0f, 1.0f);
      }
      bool escaped = false;
      if (n < a.max_bounces) {
        // (variant 13: a path's last bounce -- never its first -- needs neither the hit distance nor a next ray: pt_trace.h, pt_grid.h)
        const bool dead_end = POOLED && PT_V13_DEAD_END && (n > 0) & (n == a.max_bounces - 1);
        escaped = !bounce_once<RNG, K.tracer>(L, sc, a.n_spheres, o, d, color, mask, rng, var, n, live, live & prim_ok & (n == 0), dead_end);
        if (live) n++;
      }
      if (live & (escaped | (n >= a.max_bounces))) {
        if (!escaped) {
          L.color = L.color + color;                 // :198
          if (sc.lean && !(POOLED && PT_V13_WELFORD_TABLE)) welford_update(var[0], luminance(color)); else welford_update(var[0], luminance(color), sc.rcpn);  // :200
        }
        i++;
        n = 0;
      }
    }
    if (by_progress) __builtin_amdgcn_s_setprio(0);
  }
  if constexpr (kDecoupled) {
    // Variant 11 with the nearest-hit search and the rest of the bounce at DIFFERENT times per lane.  In variant 11 a wave
    // walks the grid until its slowest lane is done (a ray needs 7 test trips, the wave makes 21: a quarter of the lanes
    // work) and only then shades.  Here a lane keeps its walk (GridWalk) across iterations of this loop: the wave leaves the
    // walk as soon as PT_GRID_PARK of its lanes have nothing left to do, those lanes finish their search (exact step), shade,
    // start their next ray -- next bounce, or next sample: the path regeneration of variant 10 -- and join the lanes that
    // are still walking.  Shading then runs with >= PT_GRID_PARK of 64 lanes instead of 64, the walk with most lanes busy
    // instead of a quarter.  Per pixel the sequence of operations is the reference's, as in variants 10 and 11.
    int n = 0;
    F3 o = eye, d = eye;
    F3 color = mk3(0.0f, 0.0f, 0.0f), mask = mk3(1.0f, 1.0f, 1.0f);
    GridWalk w;
    w.a = 1.0f;
    w.s = Near2{0.0f, 0.0f, 0};
    w.tmax0 = w.tmax1 = w.tmax2 = w.tdel0 = w.tdel1 = w.tdel2 = 0.0f;
    w.cidx = w.cs0 = w.cs1 = w.cs2 = 0;
    w.left = w.k0 = w.k1 = w.n0 = w.n1 = 0u;
    w.have_next = w.walking = w.forced = false;
    w.e0 = w.e1 = 0u;
    w.t_box = 0.0f;
    bool in_walk = false;  // a ray's search is under way
    bool brute = false;    // ... on the brute-force path (the grid is absent or does not admit the ray)
    for (;;) {
      if (__builtin_amdgcn_ballot_w64(i < a.spp) == 0) break;
      const bool ready = (i < a.spp) & !(in_walk & !brute & w.busy());
      if (ready) {
        if (in_walk) {  // the search of the ray in hand is over: exact step, shading (:156-196)
          float t = 0.0f;
          int idx = 0;
          bool hit = false;
          if (a.n_spheres > 0) {
            if (brute) hit = intersect_scene_screened_large(sc, a.n_spheres, o, d, make_ray_const(d), t, idx);
            else hit = grid_end(w, sc, grid, a.n_spheres, o, d, t, idx);
          }
          const bool escaped = !bounce_shade<RNG, K.tracer>(L, sc, o, d, color, mask, rng, var, n, hit, t, idx);
          n++;
          if (escaped | (n >= a.max_bounces)) {
            if (!escaped) {
              L.color = L.color + color;                 // :198
              if (sc.lean) welford_update(var[0], luminance(color)); else welford_update(var[0], luminance(color), sc.rcpn);  // :200
            }
            i++;
            n = 0;
          }
          in_walk = false;
        }
        if (i < a.spp) {  // the next ray of this pixel
          if (n == 0) {  // :219-229
            rng.begin_sample((uint32_t)i);
            primary_ray(rng, d);
            o = eye;
            color = mk3(0.0f, 0.0f, 0.0f);
            mask = mk3(1.0f, 1.0f, 1.0f);
          }
          const float aa = dot(d, d);
          brute = !(grid.valid && a.n_spheres > 0 && grid_admits(grid, o, d, aa));
          if (!brute) grid_begin(w, grid, o, d, aa);
          in_walk = true;
        }
      }
      grid_trips<true>(w, grid, o, d, in_walk & !brute, i < a.spp, PT_GRID_PARK);
    }
  }
  if constexpr (K.loop == PT_LOOP_PAIRS) {
    const int draws = (a.spp != 1 ? 2 : 0) + 2 * a.max_bounces;  // consumed by a path that never escapes
    for (; i + 2 <= a.spp; i += 2) {
      Rng<RNG> g[2] = {rng, rng};
      g[0].begin_sample((uint32_t)i);
      if constexpr (RNG == PT_RNG_XORWOW) xorwow_skip(g[1].st, draws);
      g[1].begin_sample((uint32_t)i + 1u);
      F3 o2[2] = {eye, eye}, d2[2];
      primary_ray(g[0], d2[0]);
      primary_ray(g[1], d2[1]);
      PathResult res[2];
      trace_paths<RNG, 2>(res, sc, a.n_spheres, o2, d2, g, a.max_bounces);
      accumulate_path(L, var, res[0]);
      if (RNG == PT_RNG_XORWOW && __builtin_expect(res[0].escaped, 0)) {
        // A consumed fewer draws than assumed: B's stream was wrong, retrace it from A's true state
        rng = g[0];
        rng.begin_sample((uint32_t)i + 1u);
        F3 dir;
        primary_ray(rng, dir);
        trace_ray<RNG, K.tracer>(L, sc, a.n_spheres, eye, dir, rng, var, a.max_bounces);
      } else {
        accumulate_path(L, var, res[1]);
        rng = g[1];
      }
    }
  }
  if constexpr (!kRegen && !kDecoupled) {  // sample after sample (and the odd sample the pairs leave)
    // Issue priority by progress (long waves only).  A SIMD serves its waves oldest first: of four waves that start together
    // the favoured one finishes in half the time its fair share would take and the last one finishes its work alone, which a
    // lone wave cannot do at more than ~45 % of the SIMD's issue rate (a frame of 1024 workgroups x 4096 spp: first wave done
    // after 27 ms, last after 61; tools/wave_timing.py) -- and the end of EVERY kernel looks like that.  With s_setprio
    // 3, 2, 1, 0 by quarter of its own samples a wave that is ahead yields to the others on its SIMD, they reach the end
    // together, and the tail disappears (the same frame: 54 ms; the headline's four rounds: 52.4 -> 50.8 ms).  Scheduling
    // only: no value changes.  Not for short waves (the setting costs them 0.5 %; their kernels have many rounds anyway).
    const int span = i_end - i_begin;  // this workgroup's samples (all of them unless the frame is chunked)
    // ... and not for frames of many rounds of short waves.  A frame that fits the chip in ONE round (the interactive shape:
    // 512^2 x 4 spp = exactly four waves per SIMD) is all tail, however short its waves: there the priority follows the
    // sample index itself (config 5: 0.1218 -> see profiles/r03).  The launcher decides (a.prio).
    const bool by_progress = a.prio != 0u && span >= 4;
    const int q1 = i_begin + span / 4, q2 = i_begin + span / 2, q3 = i_end - span / 4;
    const int stride_mask = span >= 64 ? 15 : 0;  // how often the band is looked at
    const int i_stop = active ? i_end : i;
    for (; i < i_stop; i++) {  // :219
      if (by_progress) {
        const int iu = __builtin_amdgcn_readfirstlane(i);  // the sample index is the same in every lane that is in this loop
        if ((iu & stride_mask) == 0) {
          if (iu < q1) __builtin_amdgcn_s_setprio(3);
          else if (iu < q2) __builtin_amdgcn_s_setprio(2);
          else if (iu < q3) __builtin_amdgcn_s_setprio(1);
          else __builtin_amdgcn_s_setprio(0);
        }
      }
      rng.begin_sample((uint32_t)i);
      F3 dir;
      primary_ray(rng, dir);
      trace_ray<RNG, K.tracer, REFB, kWalls>(L, sc, a.n_spheres, eye, dir, rng, var, a.max_bounces);  // :231
    }
    if (by_progress) __builtin_amdgcn_s_setprio(0);
  }
  if constexpr (CHUNKS) {
    if (chunk + 1u < n_chunks) {  // not the last chunk: hand the pixel's state over and leave
      if (active) {
        auto st = [&](int w, uint32_t v) { a.chunk_state[(size_t)w * a.tile_pixels + tp] = v; };
        auto stf = [&](int w, float v) { st(w, __float_as_uint(v)); };
        stf(PT_REC_COLOR, L.color.x); stf(PT_REC_COLOR + 1, L.color.y); stf(PT_REC_COLOR + 2, L.color.z);
        stf(PT_REC_NORMAL, L.normal.x); stf(PT_REC_NORMAL + 1, L.normal.y); stf(PT_REC_NORMAL + 2, L.normal.z);
        stf(PT_REC_ALBEDO, L.albedo.x); stf(PT_REC_ALBEDO + 1, L.albedo.y); stf(PT_REC_ALBEDO + 2, L.albedo.z);
        stf(PT_REC_DEPTH, L.depth);
        st(PT_REC_N_COLOR, (uint32_t)var[0].n);
        st(PT_REC_N_HIT, (uint32_t)var[1].n);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          stf(PT_REC_MEAN + 2 * k, var[k].mean);
          stf(PT_REC_M2 + 2 * k, var[k].M2);
        }
        if constexpr (RNG == PT_RNG_XORWOW) {
          st(PT_REC_RNG, rng.st.d); st(PT_REC_RNG + 1, rng.st.v0); st(PT_REC_RNG + 2, rng.st.v1); st(PT_REC_RNG + 3, rng.st.v2); st(PT_REC_RNG + 4, rng.st.v3); st(PT_REC_RNG + 5, rng.st.v4);
        }
      }
      chunk_publish(a, block_id, chunk);
      return;
    }
  }

  const float fs = (float)a.spp;  // :234-237
  float px[14];
  frame_values(L, var, fs, px);  // :240-254
  float* out_f = a.out;  // this frame's buffers
  float* vtx_f = a.vertices;
  if constexpr (FRAMES) {
    out_f += (size_t)fr * args.out_stride;
    if (vtx_f) vtx_f += (size_t)fr * args.vtx_stride;
  }
  if (!ADAPTIVE && vtx_f && active) store_display_vertex(vtx_f + (size_t)tp * 3, a.width, row, col, px[0], px[1], px[2]);
  // The 64 pixels of a wave are 64 consecutive columns, so their 64 x 14 floats are ONE contiguous
  // 3584-byte span of the [row][col][14] buffer: transpose through the wave's own LDS slice and write
  // it as 224 coalesced 16-byte stores (3.5 per lane) instead of 14 strided dword stores per lane.
  if (ADAPTIVE) {
    // (an adaptive pass writes only the record: its lanes are scattered pixels; pt_adaptive.hip forms the frame)
  } else if (!REF && a.planar) {  // channel-first: consecutive lanes are consecutive columns of one plane, stores coalesce as they are
    // (the reference-configuration builds are interleaved-only: the launcher sends planar frames to the generic build)
    if (active) {
#pragma unroll
      for (int c = 0; c < 14; c++) out_f[(size_t)c * a.tile_pixels + tp] = px[c];
    }
  } else {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool wave_full = (__builtin_amdgcn_ballot_w64(active) == ~0ull) && ((reinterpret_cast<uintptr_t>(out_f) & 15u) == 0u) &&
                         K.grid == PT_GRID_NONE;  // variants 11-13: the LDS holds the grid until the last wave is done: plain stores there
  if (wave_full) {
    float* wl = reinterpret_cast<float*>(lds_scene + a.scene_lds_f4) + wave * (64 * 14);
#pragma unroll
    for (int c = 0; c < 14; c++) wl[lane * 14 + c] = px[c];
    __builtin_amdgcn_wave_barrier();  // DS operations of one wave execute in order: the reads below see these writes
    const float4* src = reinterpret_cast<const float4*>(wl);
    float4* dst = reinterpret_cast<float4*>(out_f + (size_t)(tp - (uint32_t)lane) * 14);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int q = lane + 64 * k;
      if (q < 224) dst[q] = src[q];
    }
  } else if (active) {
    float* o = out_f + (size_t)tp * 14;
#pragma unroll
    for (int c = 0; c < 14; c++) o[c] = px[c];
  }
  }
  if constexpr (FRAME_LOOP) {
    __builtin_amdgcn_wave_barrier();  // (the wave's transpose slice is reused by its next frame)
    if (++fr < fr_count) goto frame_top;
  }
  if constexpr (RESUME) {  // the pixel's state after spp samples, for the next pass (the frame above is output only)
    if (active) {
      uint32_t* rec = args.session;
      auto st = [&](int w, uint32_t v) { rec[(size_t)w * a.tile_pixels + tp] = v; };
      auto stf = [&](int w, float v) { st(w, __float_as_uint(v)); };
      stf(PT_REC_COLOR, L.color.x); stf(PT_REC_COLOR + 1, L.color.y); stf(PT_REC_COLOR + 2, L.color.z);
      stf(PT_REC_NORMAL, L.normal.x); stf(PT_REC_NORMAL + 1, L.normal.y); stf(PT_REC_NORMAL + 2, L.normal.z);
      stf(PT_REC_ALBEDO, L.albedo.x); stf(PT_REC_ALBEDO + 1, L.albedo.y); stf(PT_REC_ALBEDO + 2, L.albedo.z);
      stf(PT_REC_DEPTH, L.depth);
      st(PT_REC_N_COLOR, (uint32_t)var[0].n);
      st(PT_REC_N_HIT, (uint32_t)var[1].n);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        stf(PT_REC_MEAN + 2 * k, var[k].mean);
        stf(PT_REC_M2 + 2 * k, var[k].M2);
      }
      if constexpr (RNG == PT_RNG_XORWOW) {
        st(PT_REC_RNG, rng.st.d); st(PT_REC_RNG + 1, rng.st.v0); st(PT_REC_RNG + 2, rng.st.v1); st(PT_REC_RNG + 3, rng.st.v2); st(PT_REC_RNG + 4, rng.st.v3); st(PT_REC_RNG + 5, rng.st.v4);
      }
    }
  }

  if constexpr (RNG == PT_RNG_XORWOW) {
    if (a.rng_state && active) {  // :256
      uint32_t* s = a.rng_state + (size_t)tp * 6;
      s[0] = rng.st.d;
      s[1] = rng.st.v0;
      s[2] = rng.st.v1;
      s[3] = rng.st.v2;
      s[4] = rng.st.v3;
      s[5] = rng.st.v4;
    }
  }
  if constexpr (CHUNKS) {
    if (n_chunks > 1u) chunk_publish(a, block_id, chunk);  // count == chunks: this block's frame and generator state are complete
  }
}


// ---- variant 8: four lanes per pixel (small tiles) ----------------------------------------------
// A rank of an 8-GPU run renders 131 072 pixels = 2 waves per SIMD with one lane per pixel, which is
// latency-bound (HISTORY.md B.2).  Here lane (pixel, s) traces samples s, s+4, s+8, ... so the same tile
// has 4x the waves.  What the contract fixes -- one sequential generator per pixel, sequential float
// sums, sequential Welford updates -- is preserved:
//  * xorwow: lane s starts from the pixel's state advanced by s*D draws and skips 3*D draws after each
//    of its samples, D = 2 + 2*max_bounces being what a non-escaping path consumes (speculation);
//  * after every round the four results are exchanged through the wave's LDS slice and applied IN
//    SAMPLE ORDER, feature-parallel: lane 0 owns the colour sums + colour variance, lane 1 normal,
//    lane 2 albedo, lane 3 depth -- the same additions and Welford updates as the one-lane kernel,
//    just done by four lanes side by side;
//  * if a sample that is not the frame's last one escapes (consumed fewer draws), every later
//    speculative state of that pixel is wrong: the records after it are discarded and the group
//    continues in sequential mode (lane 0 traces, all four still accumulate) from that sample's true
//    final state.  Never happens in a closed scene; in an open one the kernel degrades to 1/4
//    efficiency for that pixel but stays exact.
// Variant 9 is the same kernel with TWO lanes per pixel, each owning two features: a third of the generator
// skip-ahead (D instead of 3 D draws per sample), for tiles that are only moderately too small -- with its reference-
// configuration build (round 3) the fastest kernel on a tile of two one-lane waves per SIMD, which it turns into ONE round of
// four (the 1/8 frame of an 8-GPU run: 6.90 ms against variant 8's 7.55 and variant 6's 8.14; pt_capi.hip, small_tile_variant).
constexpr int kRecWords = 24;  // 4 feature blocks {v0,v1,v2,x} + flags + 6 state words, padded

template <int RNG, int kSplit, bool LEAN = false, int REFB = 0>
__global__ void __launch_bounds__(PT_BLOCK_THREADS) pixel_kernel_split(PixelKernelArgs a) {
  constexpr bool REF = REFB != 0;
  constexpr VariantInfo K = kVariants[split_row(kSplit)];  // this kernel's row (variant 8 or 9)
  static_assert(K.lanes == kSplit && K.threads == PT_BLOCK_THREADS && (!REF || K.ref_builds) && (!LEAN || K.lean == PT_LEAN_BIG), "a pixel_kernel_split build is one its row announces");
  if constexpr (REF) {
    a.n_spheres = 9;
    a.max_bounces = REFB;
  }
  constexpr int kOwn = 4 / kSplit;  // features accumulated by one lane
  if constexpr (REF) {  // repair launch: only the pixel blocks a broken chunked launch left untouched (pixel_kernel)
    if (a.repair != 0u && __hip_atomic_load(a.chunk_flag + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.repair) return;
  }
  extern __shared__ float4 lds_scene[];
  SceneLds sc = stage_scene<false>(a.spheres, a.n_spheres, lds_scene, LEAN, mk3(a.eye[0], a.eye[1], a.eye[2]), a.spp);
  sc.small_only = !LEAN && (K.lean == PT_LEAN_BIG || REF);  // variant 8 has a lean build for larger scenes, variant 9 has not (its REF builds see 9 spheres)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xl = reinterpret_cast<float*>(lds_scene + a.scene_lds_f4) + wave * (64 * kRecWords);
  const int gbase = lane & ~(kSplit - 1);

  // Sample chunking as in pixel_kernel (reference-configuration builds): workgroup blockIdx.x = chunk * n_blocks + block renders
  // the samples [chunk * per, (chunk + 1) * per) of its 256 / kSplit pixels and hands their state to the next chunk through
  // chunk_state (same 26-word layout: every lane stores the features it owns, lane 0 of a pixel the true generator state).
  constexpr bool CHUNKS = K.chunk_build(REF);
  uint32_t block_id = blockIdx.x, chunk = 0u, n_chunks = 1u;
  if constexpr (CHUNKS) {
    if (a.chunks > 1u) {
      const uint32_t n_blocks = (uint32_t)(((uint64_t)a.tile_pixels * kSplit + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS);
      n_chunks = a.chunks;
      chunk = blockIdx.x / n_blocks;
      block_id = blockIdx.x - chunk * n_blocks;
    }
  }
  const uint32_t gl = block_id * PT_BLOCK_THREADS + threadIdx.x;
  const uint32_t tp = gl / kSplit;      // pixel index inside the tile
  const int s = (int)(gl % kSplit);     // sample slot; this lane accumulates features s*kOwn .. s*kOwn + kOwn - 1
  const bool active = tp < a.tile_pixels;
  const int row = a.row_begin + (int)(tp / (uint32_t)a.width);
  const int col = (int)(tp % (uint32_t)a.width);
  const uint32_t id = (uint32_t)row * (uint32_t)a.width + (uint32_t)col;

  Rng<RNG> rng;
  const int D = (a.spp != 1 ? 2 : 0) + 2 * a.max_bounces;
  if constexpr (RNG == PT_RNG_XORWOW) {
    if (a.rng_state && active) {
      const uint32_t* p = a.rng_state + (size_t)tp * 6;
      rng.st = Xorwow{p[0], p[1], p[2], p[3], p[4], p[5]};
    } else {
      xorwow_init(rng.st, (uint64_t)id + a.seed);
    }
    xorwow_skip(rng.st, s * D);
  } else {
    rng.k0 = (uint32_t)a.seed;
    rng.k1 = (uint32_t)(a.seed >> 32) ^ a.frame;
    rng.pix = id;
  }
  Xorwow final_state = Xorwow{0, 0, 0, 0, 0, 0};
  if constexpr (RNG == PT_RNG_XORWOW) final_state = rng.st;  // spp == 0 never happens; overwritten below

  const F3 B0 = mk3(a.basis[0], a.basis[1], a.basis[2]), B1 = mk3(a.basis[3], a.basis[4], a.basis[5]);
  const F3 B2 = mk3(a.basis[6], a.basis[7], a.basis[8]), B3 = mk3(a.basis[9], a.basis[10], a.basis[11]);
  const F3 eye = mk3(a.eye[0], a.eye[1], a.eye[2]);
  const bool pow2_image = ((a.width & (a.width - 1)) == 0) && ((a.height & (a.height - 1)) == 0);  // wave-uniform
  const float inv_w = 1.0f / (float)a.width, inv_h = 1.0f / (float)a.height;  // exact for powers of two

  if constexpr (REF) {
#ifndef PT_NO_FOOTPRINT
    if (a.spp >= PT_FOOTPRINT_MIN_SPP) {  // once per pixel: the spheres its primary rays can return (pt_footprint.h); the wave ranks the union
      auto dir_at = [&](float sx, float sy) {
        if (pow2_image) {
          sx *= inv_h;
          sy *= inv_w;
        } else {
          sx /= (float)a.height;
          sy /= (float)a.width;
        }
        return lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx);
      };
      const uint32_t mine = active ? primary_candidates(sc, a.n_spheres, (float)row, (float)col, dir_at) : 0u;
      uint32_t wave_mask = 0u;
#pragma unroll
      for (int j = 0; j < 9; j++) wave_mask |= (__builtin_amdgcn_ballot_w64(((mine >> j) & 1u) != 0u) != 0ull) ? (1u << j) : 0u;
      sc.prim_mask = wave_mask;
    }
#endif
  }

  float sum0[kOwn], sum1[kOwn], sum2[kOwn];  // this lane's feature sums (depth uses sum0 only)
  Welford w[kOwn];
#pragma unroll
  for (int q = 0; q < kOwn; q++) {
    sum0[q] = sum1[q] = sum2[q] = 0.0f;
    w[q] = Welford{0, 0.0f, 0.0f};
  }
  bool seq = false;  // group-uniform: sequential mode after a failed speculation
  int i_begin = 0, i_end = a.spp;  // this workgroup's samples (all of them unless the frame is chunked)
  if constexpr (CHUNKS) {
    if (n_chunks > 1u) {
      int per = (a.spp + (int)n_chunks - 1) / (int)n_chunks;
      per = (per + kSplit - 1) / kSplit * kSplit;  // whole rounds
      i_begin = (int)chunk * per < a.spp ? (int)chunk * per : a.spp;
      i_end = i_begin + per < a.spp ? i_begin + per : a.spp;
      if (chunk > 0u) {
        if (chunk_wait(a, block_id, chunk)) return;  // broken chain: nothing of the block is written (pixel_kernel)
        if (active) {
          auto ld = [&](int w) { return __hip_atomic_load(a.chunk_state + (size_t)w * a.tile_pixels + tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
          auto ldf = [&](int w) { return __uint_as_float(ld(w)); };
#pragma unroll
          for (int q = 0; q < kOwn; q++) {
            const int f = s * kOwn + q;  // 0 colour, 1 normal, 2 albedo, 3 depth
            sum0[q] = ldf(f < 3 ? PT_REC_COLOR + 3 * f : PT_REC_DEPTH);
            sum1[q] = f < 3 ? ldf(PT_REC_COLOR + 3 * f + 1) : 0.0f;
            sum2[q] = f < 3 ? ldf(PT_REC_COLOR + 3 * f + 2) : 0.0f;
            w[q] = Welford{(int)ld(f == 0 ? PT_REC_N_COLOR : PT_REC_N_HIT), ldf(PT_REC_MEAN + 2 * f), ldf(PT_REC_M2 + 2 * f)};
          }
          if constexpr (RNG == PT_RNG_XORWOW) {  // the pixel's true state after sample i_begin - 1; lane s starts s samples further on
            rng.st = Xorwow{ld(PT_REC_RNG), ld(PT_REC_RNG + 1), ld(PT_REC_RNG + 2), ld(PT_REC_RNG + 3), ld(PT_REC_RNG + 4), ld(PT_REC_RNG + 5)};
            final_state = rng.st;
            xorwow_skip(rng.st, s * D);
          }
        }
      }
    }
  }
  int base = i_begin;  // group-uniform: first sample of the current round

  // issue priority by progress, as in pixel_kernel (there: why); the progress of a wave is that of its first pixel group
  const int span = i_end - i_begin;
  const bool by_progress = a.spp >= PT_PRIO_MIN_SPP && span >= 4;
  const int q1 = i_begin + span / 4, q2 = i_begin + span / 2, q3 = i_end - span / 4;
  int last_band = -1;
  while (base < i_end) {
    if (by_progress) {
      const int bu = __builtin_amdgcn_readfirstlane(base);
      const int band = (bu >= q1 ? 1 : 0) + (bu >= q2 ? 1 : 0) + (bu >= q3 ? 1 : 0);
      if (band != last_band) {  // wave-uniform
        last_band = band;
        if (band == 0) __builtin_amdgcn_s_setprio(3);
        else if (band == 1) __builtin_amdgcn_s_setprio(2);
        else if (band == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
    }
    const int k = seq ? base : base + s;
    const bool mine = active && (!seq || s == 0) && k < i_end;
    PathResult res[1];
    res[0].color = res[0].normal0 = res[0].albedo0 = mk3(0.0f, 0.0f, 0.0f);
    res[0].t0 = 0.0f;
    res[0].hit0 = res[0].escaped = false;
    if (mine) {
      Rng<RNG> g[1] = {rng};
      g[0].begin_sample((uint32_t)k);
      float sx = (float)row, sy = (float)col;  // :221-229
      if (a.spp != 1) {
        float jx, jy;
        g[0].jitter(jx, jy);
        sx += jx * 1.0f - 0.5f;
        sy += jy * 1.0f - 0.5f;
      }
      if (pow2_image) {
        sx *= inv_h;
        sy *= inv_w;
      } else {
        sx /= (float)a.height;
        sy /= (float)a.width;
      }
      F3 o1[1] = {eye}, d1[1] = {lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx)};
      trace_paths<RNG, 1, REFB>(res, sc, a.n_spheres, o1, d1, g, a.max_bounces);
      rng = g[0];
    }
    // publish this lane's sample
    float* rec = xl + lane * kRecWords;
    const float lumC = luminance(res[0].color), lumN = luminance(res[0].normal0);
    const float lumA = sc.lean ? luminance(res[0].albedo0) : res[0].lum_albedo0;  // staged per sphere where the scene image is (pt_scene_lds.h)
    const uint32_t own_fl = (mine ? 1u : 0u) | (res[0].hit0 ? 2u : 0u) | (res[0].escaped ? 4u : 0u);
    *reinterpret_cast<float4*>(rec + 0) = make_float4(res[0].color.x, res[0].color.y, res[0].color.z, lumC);
    *reinterpret_cast<float4*>(rec + 4) = make_float4(res[0].normal0.x, res[0].normal0.y, res[0].normal0.z, lumN);
    *reinterpret_cast<float4*>(rec + 8) = make_float4(res[0].albedo0.x, res[0].albedo0.y, res[0].albedo0.z, lumA);
    *reinterpret_cast<float4*>(rec + 12) = make_float4(res[0].t0, 0.0f, 0.0f, res[0].t0);
    reinterpret_cast<uint32_t*>(rec)[16] = own_fl;
    if constexpr (RNG == PT_RNG_XORWOW) {
      uint32_t* ru = reinterpret_cast<uint32_t*>(rec) + 17;
      ru[0] = rng.st.d; ru[1] = rng.st.v0; ru[2] = rng.st.v1; ru[3] = rng.st.v2; ru[4] = rng.st.v3; ru[5] = rng.st.v4;
    }
    __builtin_amdgcn_wave_barrier();
    // apply the round's samples in order to this lane's feature
    bool failed = false;
    int consumed = 0;  // samples of this round that count (all of them unless a speculation failed)
    // Every record of every pixel group of this wave a traced sample that hit something and stayed inside (wave-uniform; in a
    // closed scene: always, except in a ragged last wave): every enable below is true, so the sums and the Welford updates
    // run unconditionally -- no selects -- and the generator state is the last record's.  Same operations in the same order.
    const bool all_hits = __builtin_amdgcn_ballot_w64(own_fl != 3u) == 0;
    if (all_hits) {
#pragma unroll
      for (int j = 0; j < kSplit; j++) {
        const float* rj = xl + (gbase + j) * kRecWords;
#pragma unroll
        for (int q = 0; q < kOwn; q++) {
          const float4 v = *reinterpret_cast<const float4*>(rj + 4 * (s * kOwn + q));
          sum0[q] = sum0[q] + v.x;
          sum1[q] = sum1[q] + v.y;
          sum2[q] = sum2[q] + v.z;
          if (sc.lean) welford_update(w[q], v.w); else welford_update(w[q], v.w, sc.rcpn);
        }
      }
      if constexpr (RNG == PT_RNG_XORWOW) {
        const uint32_t* ru = reinterpret_cast<const uint32_t*>(xl + (gbase + kSplit - 1) * kRecWords) + 17;
        final_state = Xorwow{ru[0], ru[1], ru[2], ru[3], ru[4], ru[5]};
      }
      consumed = kSplit;
    } else {
#pragma unroll
    for (int j = 0; j < kSplit; j++) {
      const float* rj = xl + (gbase + j) * kRecWords;
      const uint32_t fl = reinterpret_cast<const uint32_t*>(rj)[16];
      const bool valid = ((fl & 1u) != 0u) & !failed;
      const bool hit0 = (fl & 2u) != 0u, esc = (fl & 4u) != 0u;
#pragma unroll
      for (int q = 0; q < kOwn; q++) {
        const int f = s * kOwn + q;  // 0 colour, 1 normal, 2 albedo, 3 depth
        const float4 v = *reinterpret_cast<const float4*>(rj + 4 * f);
        const bool en_sum = valid & ((f == 0) | hit0);        // colour is always added (:159,:198); AOVs on a first hit (:187-190)
        const bool en_w = valid & ((f == 0) ? !esc : hit0);    // :200 / :192-194
        sum0[q] = en_sum ? sum0[q] + v.x : sum0[q];
        sum1[q] = en_sum ? sum1[q] + v.y : sum1[q];
        sum2[q] = en_sum ? sum2[q] + v.z : sum2[q];
        Welford wn = w[q];
        if (sc.lean) welford_update(wn, v.w); else welford_update(wn, v.w, sc.rcpn);
        w[q].n = en_w ? wn.n : w[q].n;  // field-wise: a struct select would go through scratch
        w[q].mean = en_w ? wn.mean : w[q].mean;
        w[q].M2 = en_w ? wn.M2 : w[q].M2;
      }
      if constexpr (RNG == PT_RNG_XORWOW) {
        if (valid) {
          const uint32_t* ru = reinterpret_cast<const uint32_t*>(rj) + 17;
          final_state = Xorwow{ru[0], ru[1], ru[2], ru[3], ru[4], ru[5]};
        }
        const int kj = seq ? base : base + j;
        if (valid & esc & !seq & (kj < i_end - 1)) failed = true;  // later speculative states are wrong
      }
      consumed += valid ? 1 : 0;
    }
    }
    __builtin_amdgcn_wave_barrier();  // records are rewritten next round
    if (!seq) {
      if (failed) {
        if (s == 0 && a.fail_count) atomicAdd(a.fail_count, 1u);  // lets the host stop speculating on open scenes
        seq = true;
        base += consumed;          // resume right after the escaped sample
        if constexpr (RNG == PT_RNG_XORWOW) rng.st = final_state;  // its true final state (only lane 0 traces from here on)
      } else {
        base += kSplit;
        if constexpr (RNG == PT_RNG_XORWOW) {
          // (reference-configuration builds: the step count is a compile-time constant unless the frame has one sample per pixel)
          if (REFB != 0 && a.spp != 1) xorwow_skip_n<(kSplit - 1) * (2 + 2 * (REFB != 0 ? REFB : 1))>(rng.st);
          else xorwow_skip(rng.st, (kSplit - 1) * D);
        }
      }
    } else {
      base += 1;
      if constexpr (RNG == PT_RNG_XORWOW) rng.st = final_state;
    }
  }
  if (by_progress) __builtin_amdgcn_s_setprio(0);

  if constexpr (CHUNKS) {
    if (chunk + 1u < n_chunks) {  // not the last chunk: hand the pixel's state over and leave
      if (active) {
        auto st = [&](int wd, uint32_t v) { a.chunk_state[(size_t)wd * a.tile_pixels + tp] = v; };
        auto stf = [&](int wd, float v) { st(wd, __float_as_uint(v)); };
#pragma unroll
        for (int q = 0; q < kOwn; q++) {
          const int f = s * kOwn + q;
          if (f < 3) {
            stf(PT_REC_COLOR + 3 * f, sum0[q]); stf(PT_REC_COLOR + 3 * f + 1, sum1[q]); stf(PT_REC_COLOR + 3 * f + 2, sum2[q]);
          } else {
            stf(PT_REC_DEPTH, sum0[q]);
          }
          if (f < 2) st(PT_REC_N_COLOR + f, (uint32_t)w[q].n);  // the three first-hit accumulators count together: the normal's stands for them (PT_REC_N_HIT)
          stf(PT_REC_MEAN + 2 * f, w[q].mean);
          stf(PT_REC_M2 + 2 * f, w[q].M2);
        }
        if constexpr (RNG == PT_RNG_XORWOW) {
          if (s == 0) {
            st(PT_REC_RNG, final_state.d); st(PT_REC_RNG + 1, final_state.v0); st(PT_REC_RNG + 2, final_state.v1); st(PT_REC_RNG + 3, final_state.v2); st(PT_REC_RNG + 4, final_state.v3); st(PT_REC_RNG + 5, final_state.v4);
          }
        }
      }
      chunk_publish(a, block_id, chunk);
      return;
    }
  }

  if (active) {  // :234-254, each lane stores its feature
    const float fs = (float)a.spp;
    // channel c of this pixel: interleaved [row][col][14] or channel-first [14][tile pixels]
    const bool planar = !REF && a.planar;
    float* o = planar ? a.out + tp : a.out + (size_t)tp * 14;
    const size_t cs = planar ? (size_t)a.tile_pixels : 1;
#pragma unroll
    for (int q = 0; q < kOwn; q++) {
      const int f = s * kOwn + q;
      if (f < 3) {
        const float v0 = sum0[q] / fs, v1 = sum1[q] / fs, v2 = sum2[q] / fs;
        o[(3 * f + 0) * cs] = v0;
        o[(3 * f + 1) * cs] = v1;
        o[(3 * f + 2) * cs] = v2;
        if (f == 0 && a.vertices) store_display_vertex(a.vertices + (size_t)tp * 3, a.width, row, col, v0, v1, v2);  // the colour's owner
      } else {
        o[9 * cs] = sum0[q] / fs;
      }
      o[(10 + f) * cs] = welford_variance(w[q]);
    }
    if constexpr (RNG == PT_RNG_XORWOW) {
      if (a.rng_state && s == 0) {  // :256
        uint32_t* p = a.rng_state + (size_t)tp * 6;
        p[0] = final_state.d; p[1] = final_state.v0; p[2] = final_state.v1;
        p[3] = final_state.v2; p[4] = final_state.v3; p[5] = final_state.v4;
      }
    }
  }
  if constexpr (CHUNKS) {
    if (n_chunks > 1u) chunk_publish(a, block_id, chunk);  // count == chunks: this block is complete
  }
}

// setup_random: src/pathtrace.cu:259-266
__global__ void __launch_bounds__(PT_BLOCK_THREADS)
    setup_random_kernel(uint32_t* state, int width, int row_begin, uint32_t tile_pixels, uint64_t seed) {
  const uint32_t tp = blockIdx.x * PT_BLOCK_THREADS + threadIdx.x;
  if (tp >= tile_pixels) return;
  const uint32_t id = (uint32_t)(row_begin + (int)(tp / (uint32_t)width)) * (uint32_t)width + tp % (uint32_t)width;
  Xorwow s;
  xorwow_init(s, (uint64_t)id + seed);
  uint32_t* p = state + (size_t)tp * 6;
  p[0] = s.d;
  p[1] = s.v0;
  p[2] = s.v1;
  p[3] = s.v2;
  p[4] = s.v3;
  p[5] = s.v4;
}

}  // namespace pt

// ---- launchers (host) ---------------------------------------------------------------------
#include <utility>

const VariantInfo& pt_kernel_variant(int variant) { return (variant >= 0 && variant < kNumVariants) ? kVariants[variant] : kNoVariant; }
int pt_kernel_num_variants(void) { return kNumVariants; }
int pt_kernel_block_threads(int variant) { return pt_kernel_variant(variant).threads; }
bool pt_kernel_has_variant(int variant) { return variant >= 0 && variant < kNumVariants && (PT_BUILD_EXPERIMENTS || kVariants[variant].product); }
bool pt_kernel_has_resume(int variant) { return pt_kernel_variant(variant).resume; }

// LDS layout of a launch (pt_scene_lds.h): many-sphere scenes keep only the geometry in LDS
// (variants 6, 8 and 10 -- the ones the automatic policy uses -- are also built for that layout)
static inline bool lds_lean(int n, const VariantInfo& v) { return v.lean == PT_LEAN_ALWAYS || (v.lean == PT_LEAN_BIG && n > PT_SCREEN_MAX_SPHERES); }
static inline size_t scene_lds_f4(int n, const VariantInfo& v) {
  if (lds_lean(n, v)) return pt::kTablesF4;  // the lean builds read the caller's array directly: only the small tables
  return (size_t)n * 4 + pt::kTablesF4 +  // geometry, two material slots, the eye image, the unit-length table, the wall block (variant 6)
         (v.lds_extra == PT_LDS_PACKED ? (size_t)((n + 1) / 2) * 2 : v.lds_extra == PT_LDS_WALLS ? (size_t)pt::kWallF4 : 0);
}
// what follows the scene image: one 64 x 14 float transpose slice per wave for the epilogue, or the
// split kernels' exchange records
static inline size_t tail_lds_bytes(int n, const VariantInfo& v) {
  if (v.grid == PT_GRID_LANE) return n <= pt::kGridMaxSpheres ? pt::grid_lds_bytes(n, false) : 64;  // geometry + grid tables instead of the epilogue slice
  if (v.grid == PT_GRID_POOLED)  // + per wave the test ring and the owners' result slots
    return (n <= pt::kGridMaxSpheres ? ((pt::grid_lds_bytes(n, true, v.threads) + 15) & ~(size_t)15) : 64) + (v.threads / 64) * pt::kPoolWaveBytes;
  if (v.split()) return (PT_BLOCK_THREADS / 64) * 64 * pt::kRecWords * sizeof(float);
  return (PT_BLOCK_THREADS / 64) * 64 * 14 * sizeof(float);
}
static inline size_t scene_lds_bytes(int n, const VariantInfo& v) { return scene_lds_f4(n, v) * sizeof(float4) + tail_lds_bytes(n, v); }
size_t pt_kernel_lds_bytes(int n_spheres, int variant) { return scene_lds_bytes(n_spheres, pt_kernel_variant(variant)); }

// the bounce cap of the reference-configuration build these launch parameters run (5 or 8), 0 = a generic build
static inline int ref_config(int n, int max_bounces, const VariantInfo& v, bool planar) {
  return (n == 9 && (max_bounces == 5 || max_bounces == 8) && !planar && v.ref_builds) ? max_bounces : 0;
}
int pt_kernel_ref_bounces(int n_spheres, int max_bounces, int variant, bool planar) { return ref_config(n_spheres, max_bounces, pt_kernel_variant(variant), planar); }

// ---- the selector: which build of pixel_kernel / pixel_kernel_split a launch runs ------------------------------------------------
// A flavour is the plain kernel, FRAMES (a batch), RESUME (a progressive pass) or RESUME + ADAPTIVE (... over a list of pixels).
template <bool FRAMES, bool RESUME, bool ADAPTIVE>
using kernel_fn = void (*)(typename pt::KernelArgsOf<FRAMES, RESUME, ADAPTIVE>::type);

template <bool FRAMES, bool RESUME, bool ADAPTIVE, int RNG, int VAR, bool LEAN, int REFB>
static kernel_fn<FRAMES, RESUME, ADAPTIVE> kernel_build() {
  constexpr VariantInfo v = kVariants[VAR];
  if constexpr (v.split()) return pt::pixel_kernel_split<RNG, v.lanes, LEAN, REFB>;
  else return pt::pixel_kernel<RNG, v.kernel, LEAN, REFB, FRAMES, v.wide, RESUME, ADAPTIVE>;  // (a wide row: its kernel's build with WIDE)
}

// Variant VAR's build of one flavour for a launch's LDS layout and reference configuration, or null.  Only the builds the row
// announces are instantiated, so a library holds exactly them (libptcore.so: the product variants only).
template <bool FRAMES, bool RESUME, bool ADAPTIVE, int RNG, int VAR>
static kernel_fn<FRAMES, RESUME, ADAPTIVE> variant_kernel(bool lean, int ref) {
  constexpr VariantInfo v = kVariants[VAR];
  if constexpr ((v.product || PT_BUILD_EXPERIMENTS) && (!RESUME || v.resume) && (!FRAMES || v.frames)) {
    if constexpr (v.ref_builds) {
      if (ref == 5 && !lean) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 5>();
      if (ref == 8 && !lean) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 8>();
    }
    if constexpr (!FRAMES) {  // (a batch has builds for the reference configurations only)
      if constexpr (v.lean != PT_LEAN_NEVER) {
        if (lean) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, true, 0>();
      }
      if constexpr (v.lean != PT_LEAN_ALWAYS) {
        if (!lean) return kernel_build<FRAMES, RESUME, ADAPTIVE, RNG, VAR, false, 0>();
      }
    }
  }
  return nullptr;
}

template <bool FRAMES, bool RESUME, bool ADAPTIVE, int RNG, int... VAR>
static kernel_fn<FRAMES, RESUME, ADAPTIVE> select_kernel_of(int variant, bool lean, int ref, std::integer_sequence<int, VAR...>) {
  static constexpr kernel_fn<FRAMES, RESUME, ADAPTIVE> (*of[])(bool, int) = {variant_kernel<FRAMES, RESUME, ADAPTIVE, RNG, VAR>...};
  return (variant >= 0 && variant < kNumVariants) ? of[variant](lean, ref) : nullptr;
}

// variant 12's loop assumes every ray is searched for: without bounces it runs variant 11's kernel.  (A rule about a launch's
// max_bounces, not a property of a build: the one place outside the table that names variants.)
static inline int run_variant(int variant, int max_bounces) { return (variant == 12 && max_bounces < 1) ? 11 : variant; }

template <bool FRAMES = false, bool RESUME = false, bool ADAPTIVE = false>
static kernel_fn<FRAMES, RESUME, ADAPTIVE> select_kernel(int rng_mode, int variant, int n_spheres, int max_bounces, bool planar) {
  const VariantInfo& v = pt_kernel_variant(variant);
  const bool lean = lds_lean(n_spheres, v);
  const int ref = ref_config(n_spheres, max_bounces, v, planar);
  const std::make_integer_sequence<int, kNumVariants> all;
  return rng_mode == PT_RNG_PHILOX ? select_kernel_of<FRAMES, RESUME, ADAPTIVE, PT_RNG_PHILOX>(variant, lean, ref, all)
                                   : select_kernel_of<FRAMES, RESUME, ADAPTIVE, PT_RNG_XORWOW>(variant, lean, ref, all);
}

// the function a launch with these parameters runs (pt_renderer_kernel_info and the tools), null = there is no such build
const void* pt_kernel_symbol(int rng_mode, int variant, int n_spheres, int max_bounces, bool planar) {
  return (const void*)select_kernel<>(rng_mode, run_variant(variant, max_bounces), n_spheres, max_bounces, planar);
}
const void* pt_resume_kernel_symbol(int rng_mode, int variant, int n_spheres, int max_bounces, bool planar) {
  return (const void*)select_kernel<false, true>(rng_mode, variant, n_spheres, max_bounces, planar);
}
const void* pt_adaptive_kernel_symbol(int rng_mode, int variant, int n_spheres, int max_bounces, bool planar) {
  return (const void*)select_kernel<false, true, true>(rng_mode, variant, n_spheres, max_bounces, planar);
}

#ifdef PT_SCREEN_STATS
extern "C" int pt_debug_screen_stats(unsigned long long out[8], int reset) {
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pt::g_screen_stats), sizeof(zero)) != hipSuccess) return -2;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(pt::g_screen_stats), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
#endif

#ifdef PT_GRID_STATS
extern "C" int pt_debug_grid_hist(unsigned long long out[256], int reset) {
  static unsigned long long zero[256];
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pt::g_grid_hist), sizeof(zero)) != hipSuccess) return -2;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(pt::g_grid_hist), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
extern "C" int pt_debug_grid_stats(unsigned long long out[8], int reset) {
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pt::g_grid_stats), sizeof(zero)) != hipSuccess) return -2;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(pt::g_grid_stats), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
#endif

size_t pt_kernel_accel_bytes(void) { return pt::kGridAccelBytes; }

int pt_kernel_max_spheres(int variant) {
  // variants with a lean build stage nothing for big scenes; the others are bounded by their LDS image
  const VariantInfo& v = pt_kernel_variant(variant);
  if (v.lean != PT_LEAN_NEVER) return 1 << 26;  // byte offsets of the 40-byte records stay inside 32 bits
  const size_t fixed = tail_lds_bytes(0, v) + pt::kTablesF4 * sizeof(float4);
  if (v.lds_extra == PT_LDS_PACKED) return (int)((PT_LDS_BUDGET_BYTES - fixed - 2 * sizeof(float4)) / (5 * sizeof(float4)));
  return (int)((PT_LDS_BUDGET_BYTES - fixed) / (4 * sizeof(float4)));
}

hipError_t pt_launch_build_grid(const pt_sphere* spheres, int n, uint32_t* accel, const float* eye, bool pooled, hipStream_t stream, int threads) {
  // (table entries the LDS image of the kernel that will walk this grid has room for)
  hipLaunchKernelGGL(pt::build_grid_kernel, dim3(1), dim3(pt::kGridBuildThreads), 0, stream, spheres, n, accel, eye ? eye[0] : 0.0f,
                     eye ? eye[1] : 0.0f, eye ? eye[2] : 0.0f, eye ? 1 : 0, pt::grid_max_entries(n, pooled, threads));
  return hipGetLastError();
}

// where the parts of the builder's image lie (lab diagnostics: pt_debug_grid_image)
void pt_kernel_grid_layout(int n_spheres, int threads, uint64_t out[8]) {
  out[0] = pt::kGridAccelBytes;
  out[1] = pt::kGridBigOff;
  out[2] = pt::kGridStartOff;
  out[3] = pt::kGridItemsOff;
  out[4] = pt::kGridCellsOff;
  out[5] = pt::kGridEmisOff;
  out[6] = (uint64_t)pt::kGridMaxCells;
  out[7] = (uint64_t)pt::grid_max_entries(n_spheres, true, threads);
}

// does a launch with these arguments chain a pixel's samples through several workgroups (sample chunking)?
bool pt_kernel_chunked(int variant, int n_spheres, int max_bounces, bool planar, int spp, uint32_t chunks) {
  const VariantInfo& v = pt_kernel_variant(variant);
  const bool build_chunks = v.chunk_build(!lds_lean(n_spheres, v) && ref_config(n_spheres, max_bounces, v, planar));  // (what the kernel was compiled by)
  return build_chunks && chunks > 1u && chunks <= (uint32_t)PT_CHUNKS_MAX && spp >= 2 * (int)chunks &&
         (spp + (int)chunks - 1) / (int)chunks <= (v.chunk_family == PT_CHUNK_GRID ? PT_CHUNK_MAX_SAMPLES_GRID : PT_CHUNK_MAX_SAMPLES);
}

// What every launch of a pixel kernel does first: fill scene_lds_f4 and the issue priority (`samples` = the samples per pixel this
// launch renders), check the LDS budget, opt in to large dynamic LDS, enqueue the grid build of a grid variant.  Leaves the
// launch's geometry in *s.
struct LaunchShape {
  unsigned block, blocks;  // workgroup size, workgroups of one pass over the tile
  size_t lds;
};
static hipError_t prepare_launch(const void* fn, const VariantInfo& v, PixelKernelArgs& b, int samples, hipStream_t stream, LaunchShape* s) {
  if (!fn) return hipErrorInvalidValue;
  b.scene_lds_f4 = (uint32_t)scene_lds_f4(b.n_spheres, v);
  b.prio = (samples >= PT_PRIO_MIN_SPP || b.prio != 0u) ? 1u : 0u;  // long waves always; short ones when the caller says the frame is one round
  s->lds = scene_lds_bytes(b.n_spheres, v);
  const size_t lds_budget = v.wide ? (size_t)PT_LDS_WIDE_BUDGET_BYTES : (size_t)PT_LDS_BUDGET_BYTES;
  if (s->lds > lds_budget) return hipErrorInvalidValue;
  if (s->lds > 64 * 1024) {  // beyond the default dynamic-LDS limit: opt in (gfx950 has 160 KiB per CU)
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_budget);
    if (e != hipSuccess) return e;
  }
  if (v.grid != PT_GRID_NONE) {  // this launch's grid (the scene may have changed since the last one), in the renderer's scratch
    if (!b.accel) return hipErrorInvalidValue;
    hipError_t e = pt_launch_build_grid(b.spheres, b.n_spheres, const_cast<uint32_t*>(b.accel), b.eye, v.grid == PT_GRID_POOLED, stream, v.threads);
    if (e != hipSuccess) return e;
  }
  s->block = (unsigned)v.threads;
  s->blocks = (unsigned)(((uint64_t)b.tile_pixels * (uint64_t)v.lanes + s->block - 1) / s->block);
  return hipSuccess;
}

#if PT_BUILD_EXPERIMENTS
// what a launch was, for the census: from the arguments the kernel got.  `ref`: a reference-configuration build (the ones with the
// footprint analysis), `samples`: the count that build compares with PT_FOOTPRINT_MIN_SPP (pixel_kernel: pass_spp; split: a.spp)
static inline uint32_t census_modes(const PixelKernelArgs& b, bool ref, int samples) {
  return (b.chunks > 1u ? PT_CENSUS_MODE_CHUNKED : 0u) | (b.repair != 0u ? PT_CENSUS_MODE_REPAIR : 0u) | (b.planar != 0u ? PT_CENSUS_MODE_PLANAR : 0u) |
         (b.vertices ? PT_CENSUS_MODE_VERTICES : 0u) | (b.rng_state ? PT_CENSUS_MODE_RNG_STATE : 0u) |
         (ref && samples >= PT_FOOTPRINT_MIN_SPP ? PT_CENSUS_MODE_FOOTPRINT : 0u) | (b.prio != 0u ? PT_CENSUS_MODE_PRIO : 0u);
}
#endif

hipError_t pt_launch_pixel_kernel(const PixelKernelArgs& a, int rng_mode, int variant, hipStream_t stream) {
  variant = run_variant(variant, a.max_bounces);
  const auto fn = select_kernel<>(rng_mode, variant, a.n_spheres, a.max_bounces, a.planar != 0u);
  PixelKernelArgs b = a;
  LaunchShape s;
  hipError_t e = prepare_launch((const void*)fn, pt_kernel_variant(variant), b, a.spp, stream, &s);
  if (e != hipSuccess) return e;
  // sample chunking: only the reference-configuration builds of variant 6 and variant 13 hand a pixel's state from workgroup to workgroup
  const bool chunked = a.repair == 0u && pt_kernel_chunked(variant, a.n_spheres, a.max_bounces, a.planar != 0u, a.spp, a.chunks) && a.chunk_state && a.chunk_flag;
  if (a.repair != 0u && !a.chunk_flag) return hipErrorInvalidValue;  // a repair launch reads the flags its chunked predecessor left
  b.chunks = chunked ? a.chunks : 0u;
  unsigned grid = s.blocks;
  if (chunked) {
    e = hipMemsetAsync(a.chunk_flag, 0, (size_t)grid * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    grid *= a.chunks;
  }
  hipLaunchKernelGGL(fn, dim3(grid), dim3(s.block), s.lds, stream, b);
  return PT_LAUNCHED(fn, census_modes(b, ref_config(a.n_spheres, a.max_bounces, pt_kernel_variant(variant), a.planar != 0u) != 0, a.spp));
}

bool pt_kernel_has_frames(int variant, int n_spheres, int max_bounces, bool planar) {
  const VariantInfo& v = pt_kernel_variant(variant);
  return v.frames && ref_config(n_spheres, max_bounces, v, planar) != 0;
}

// XORWOW: one workgroup per pixel block, looping over the batch's frames; philox: one per (frame, pixel block) (pixel_kernel, FRAMES)
hipError_t pt_launch_frames_kernel(const FramesKernelArgs& fa, int rng_mode, int variant, hipStream_t stream) {
  const PixelKernelArgs& a = fa.base;
  if (!pt_kernel_has_frames(variant, a.n_spheres, a.max_bounces, a.planar != 0u) || fa.frames < 2u || fa.frames > (uint32_t)PT_FRAMES_MAX) return hipErrorInvalidValue;
  const auto fn = select_kernel<true>(rng_mode, variant, a.n_spheres, a.max_bounces, a.planar != 0u);
  FramesKernelArgs b = fa;
  b.base.chunks = 0u;
  b.base.repair = 0u;
  LaunchShape s;
  const hipError_t e = prepare_launch((const void*)fn, pt_kernel_variant(variant), b.base, a.spp, stream, &s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(rng_mode == PT_RNG_PHILOX ? s.blocks * fa.frames : s.blocks), dim3(s.block), s.lds, stream, b);
  return PT_LAUNCHED(fn, census_modes(b.base, true, a.spp));  // (a batch has reference-configuration builds only)
}

hipError_t pt_launch_setup_random(uint32_t* state, int width, int row_begin, uint32_t tile_pixels, uint64_t seed,
                                  hipStream_t stream) {
  const unsigned grid = (tile_pixels + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS;
  hipLaunchKernelGGL(pt::setup_random_kernel, dim3(grid), dim3(PT_BLOCK_THREADS), 0, stream, state, width, row_begin,
                     tile_pixels, seed);
  return hipGetLastError();
}

// ---- progressive passes (pixel_kernel, RESUME) ------------------------------------------------
// One pass: pt_launch_pixel_kernel without sample chunking (ra.base.chunks and repair are ignored) and with the issue priority
// decided by the pass's own sample count.  An adaptive pass launches the tile's full block count: the workgroups past the
// device-side list length leave at once (pixel_kernel, ADAPTIVE), so nothing is read back.
template <bool ADAPTIVE, class Args>
static hipError_t launch_pass(const Args& ra, int rng_mode, int variant, hipStream_t stream) {
  const PixelKernelArgs& a = ra.base;
  if (!pt_kernel_has_resume(variant) || !ra.session || ra.sample_begin < 0 || ra.sample_begin >= a.spp || a.rng_state) return hipErrorInvalidValue;
  const auto fn = select_kernel<false, true, ADAPTIVE>(rng_mode, variant, a.n_spheres, a.max_bounces, a.planar != 0u);
  Args b = ra;
  b.base.chunks = 0u;
  b.base.chunk_state = nullptr;
  b.base.chunk_flag = nullptr;
  b.base.repair = 0u;
  LaunchShape s;
  const hipError_t e = prepare_launch((const void*)fn, pt_kernel_variant(variant), b.base, a.spp - ra.sample_begin, stream, &s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(s.blocks), dim3(s.block), s.lds, stream, b);
  return PT_LAUNCHED(fn, census_modes(b.base, ref_config(a.n_spheres, a.max_bounces, pt_kernel_variant(variant), a.planar != 0u) != 0, a.spp - ra.sample_begin) |
                             (ra.sample_begin == 0 ? (uint32_t)PT_CENSUS_MODE_FIRST_PASS : 0u));
}

hipError_t pt_launch_resume_kernel(const ResumeKernelArgs& ra, int rng_mode, int variant, hipStream_t stream) {
  return launch_pass<false>(ra, rng_mode, variant, stream);
}

hipError_t pt_launch_adaptive_kernel(const AdaptiveKernelArgs& aa, int rng_mode, int variant, hipStream_t stream) {
  if (!aa.list || !aa.list_len) return hipErrorInvalidValue;
  return launch_pass<true>(aa, rng_mode, variant, stream);
}

#if PT_BUILD_EXPERIMENTS
// ---- lab library: the builds behind the selectors and the launch census (include/ptcore_lab.h) ------------------------------
// Every distinct function select_kernel<> and the fast mode's selector can return, found by walking the selectors themselves
// over (flavour, generator, row, LDS layout, reference configuration): what a row announces but the selector does not hand out
// is not here, and the tests compare this list with the rows (tests/test_kernel_census_host.py).
#include <atomic>
#include <mutex>

#include "pt_internal.h"
#include "../../include/ptcore_lab.h"

namespace {
struct CensusBuild {
  const void* fn;
  int32_t info[PT_BUILD_INFO_WORDS];  // flavour, generator, kernel row, wide, lean, reference bounces, lanes per pixel, first row that selects it
};
constexpr int kCensusMax = 256;
CensusBuild g_builds[kCensusMax];
int g_n_builds = 0;
std::atomic<uint32_t> g_launches[kCensusMax], g_modes[kCensusMax];
std::atomic<uint32_t> g_unknown_launches{0u};  // launches of a function the walk did not find (none, or the walk is wrong)
std::once_flag g_census_once;

template <bool FRAMES, bool RESUME, bool ADAPTIVE>
const void* build_of(int rng, int row, bool lean, int ref) {
  const std::make_integer_sequence<int, kNumVariants> all;
  return rng == PT_RNG_PHILOX ? (const void*)select_kernel_of<FRAMES, RESUME, ADAPTIVE, PT_RNG_PHILOX>(row, lean, ref, all)
                              : (const void*)select_kernel_of<FRAMES, RESUME, ADAPTIVE, PT_RNG_XORWOW>(row, lean, ref, all);
}

void census_add(const void* fn, int flavour, int rng, int kernel, int wide, int lean, int ref, int lanes, int row) {
  if (!fn) return;
  for (int i = 0; i < g_n_builds; i++)
    if (g_builds[i].fn == fn) return;  // (equal pointers: one build)
  if (g_n_builds >= kCensusMax) return;
  g_builds[g_n_builds++] = CensusBuild{fn, {flavour, rng, kernel, wide, lean, ref, lanes, row}};
}

void census_enumerate() {
  static const int refs[3] = {0, 5, 8};
  for (int flavour = 0; flavour < 4; flavour++)
    for (int rng = 0; rng < 2; rng++)
      for (int row = 0; row < kNumVariants; row++)
        for (int lean = 0; lean < 2; lean++)
          for (int ref : refs) {
            const VariantInfo& v = kVariants[row];
            const void* fn = flavour == 0 ? build_of<false, false, false>(rng, row, lean != 0, ref)
                           : flavour == 1 ? build_of<true, false, false>(rng, row, lean != 0, ref)
                           : flavour == 2 ? build_of<false, true, false>(rng, row, lean != 0, ref)
                                          : build_of<false, true, true>(rng, row, lean != 0, ref);
            census_add(fn, flavour, rng, v.kernel, v.wide ? 1 : 0, lean, ref, v.lanes, row);
          }
  for (int rng = 0; rng < 2; rng++) {  // the fast mode (pt_fast.hip): the reference's configuration as constants, and the generic build
    census_add(pt_fast_kernel_symbol(rng, 9, 5), 4, rng, PT_VARIANT_FAST, 0, 0, 5, 1, PT_VARIANT_FAST);
    census_add(pt_fast_kernel_symbol(rng, 1, 1), 4, rng, PT_VARIANT_FAST, 0, 0, 0, 1, PT_VARIANT_FAST);
  }
}
}  // namespace

hipError_t pt_census_launched(const void* fn, uint32_t modes) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  std::call_once(g_census_once, census_enumerate);
  for (int i = 0; i < g_n_builds; i++)
    if (g_builds[i].fn == fn) {
      g_launches[i].fetch_add(1u, std::memory_order_relaxed);
      g_modes[i].fetch_or(modes, std::memory_order_relaxed);
      return e;
    }
  g_unknown_launches.fetch_add(1u, std::memory_order_relaxed);
  return e;
}

extern "C" int pt_debug_kernel_builds(int index, int* n_builds, int32_t info[PT_BUILD_INFO_WORDS]) {
  std::call_once(g_census_once, census_enumerate);
  if (n_builds) *n_builds = g_n_builds;
  if (!info) return PT_OK;  // (only the count)
  if (index < 0 || index >= g_n_builds) return pt_fail(PT_EINVAL, "pt_debug_kernel_builds: index %d of %d builds", index, g_n_builds);
  for (int k = 0; k < PT_BUILD_INFO_WORDS; k++) info[k] = g_builds[index].info[k];
  return PT_OK;
}

extern "C" int pt_debug_variant_row(int row, int* n_rows, int32_t info[PT_ROW_INFO_WORDS]) {
  if (n_rows) *n_rows = kNumVariants;
  if (!info) return PT_OK;
  if (row < 0 || row >= kNumVariants) return pt_fail(PT_EINVAL, "pt_debug_variant_row: row %d of %d", row, kNumVariants);
  const VariantInfo& v = kVariants[row];
  const int32_t words[PT_ROW_INFO_WORDS] = {v.product, v.lanes, v.threads, v.lean, v.grid, v.wide, v.ref_builds, v.resume, v.frames, v.can_chunk, v.kernel, v.chunk_family};
  for (int k = 0; k < PT_ROW_INFO_WORDS; k++) info[k] = words[k];
  return PT_OK;
}

extern "C" int pt_debug_launch_census(int index, uint32_t* launches, uint32_t* modes) {
  std::call_once(g_census_once, census_enumerate);
  if (!launches || !modes) return pt_fail(PT_EINVAL, "pt_debug_launch_census: NULL argument");
  if (index == -1) {  // launches of functions that are not in the list of builds
    *launches = g_unknown_launches.load(std::memory_order_relaxed);
    *modes = 0u;
    return PT_OK;
  }
  if (index < 0 || index >= g_n_builds) return pt_fail(PT_EINVAL, "pt_debug_launch_census: index %d of %d builds", index, g_n_builds);
  *launches = g_launches[index].load(std::memory_order_relaxed);
  *modes = g_modes[index].load(std::memory_order_relaxed);
  return PT_OK;
}

extern "C" int pt_debug_launch_census_reset(void) {
  for (int i = 0; i < kCensusMax; i++) {
    g_launches[i].store(0u, std::memory_order_relaxed);
    g_modes[i].store(0u, std::memory_order_relaxed);
  }
  g_unknown_launches.store(0u, std::memory_order_relaxed);
  return PT_OK;
}

// ---- lab library: the two primary-ray exclusion analyses on their own (pt_debug_primary_masks / pt_debug_primary_lists) -------
// The pictures say little about them (8-16 random rays per pixel do not notice a footprint radius three times too small), so
// the tests take each lane's OWN result and hold it to a NumPy model bit for bit (tests/test_primary_exclusion_gpu.py).
namespace pt {

// A COPY of the pixel kernels' dir_at (pixel_kernel, pixel_kernel_split, pt_fast.hip: a lambda in each).  Moving the lambdas into
// one functor is not guaranteed to leave the shipped kernels' instruction streams alone, so they stay as they are; what ties this
// copy to them is the dump's `dirs` output, which the tests compare with the primary-ray formula bit for bit.
struct PrimaryDirAt {
  F3 B0, B1, B2, B3;
  float inv_w, inv_h, fw, fh;
  bool pow2_image;
  __device__ __forceinline__ explicit PrimaryDirAt(const PrimaryDumpArgs& a)
      : B0(mk3(a.basis[0], a.basis[1], a.basis[2])), B1(mk3(a.basis[3], a.basis[4], a.basis[5])),
        B2(mk3(a.basis[6], a.basis[7], a.basis[8])), B3(mk3(a.basis[9], a.basis[10], a.basis[11])),
        inv_w(1.0f / (float)a.width), inv_h(1.0f / (float)a.height), fw((float)a.width), fh((float)a.height),
        pow2_image(((a.width & (a.width - 1)) == 0) && ((a.height & (a.height - 1)) == 0)) {}
  __device__ __forceinline__ F3 operator()(float sx, float sy) const {
    if (pow2_image) {
      sx *= inv_h;
      sy *= inv_w;
    } else {
      sx /= fh;
      sy /= fw;
    }
    return lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx);
  }
};

// one lane per tile pixel, in the pixel kernels' order; the scene staged as the reference-configuration builds stage it
__global__ void __launch_bounds__(PT_BLOCK_THREADS) primary_masks_dump_kernel(PrimaryDumpArgs a, uint32_t* __restrict__ masks,
                                                                              float* __restrict__ dirs) {
  extern __shared__ float4 lds_scene[];
  const SceneLds sc = stage_scene<false>(a.spheres, a.n_spheres, lds_scene, false, mk3(a.eye[0], a.eye[1], a.eye[2]), 0);
  const uint32_t tp = blockIdx.x * PT_BLOCK_THREADS + threadIdx.x;
  if (tp >= a.tile_pixels) return;  // (after the staging barrier)
  const int row = a.row_begin + (int)(tp / (uint32_t)a.width);
  const int col = (int)(tp % (uint32_t)a.width);
  const PrimaryDirAt dir_at(a);
  masks[tp] = primary_candidates(sc, a.n_spheres, (float)row, (float)col, dir_at);  // the lane's own word, not the wave's union
  if (dirs) {
    float* out = dirs + (size_t)tp * 15;
    for (int k = 0; k < 5; k++) {  // the centre, then the four corners in the analyses' order
      const F3 d = k == 0 ? dir_at((float)row, (float)col)
                          : dir_at((float)row + (((k - 1) & 1) ? 0.5f : -0.5f), (float)col + (((k - 1) & 2) ? 0.5f : -0.5f));
      out[3 * k] = d.x;
      out[3 * k + 1] = d.y;
      out[3 * k + 2] = d.z;
    }
  }
}

// `THREADS` lanes per workgroup with the pooled kernel's LDS layout (the small tables' room, the grid image, a test pool per wave)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) primary_lists_dump_kernel(PrimaryDumpArgs a, const uint32_t* __restrict__ accel,
                                                                     uint32_t* __restrict__ lists) {
  extern __shared__ float4 lds_scene[];
  float4* image = lds_scene + kTablesF4;
  const GridLds grid = stage_grid<true>(a.spheres, a.n_spheres, accel, image);
  if (!grid.valid) return;  // (the host launches only on a valid grid)
  void* pool = reinterpret_cast<char*>(image) + ((grid_lds_bytes(a.n_spheres, true, THREADS) + 15) & ~(size_t)15);
  const uint32_t lane_id = blockIdx.x * THREADS + threadIdx.x;
  const bool active = lane_id < a.tile_pixels;  // lanes past the tile stay for the cooperative parts, as in the pixel kernels
  const int row = a.row_begin + (int)(lane_id / (uint32_t)a.width);
  const int col = (int)(lane_id % (uint32_t)a.width);
  const PrimaryDirAt dir_at(a);
  int k = 0;
  const uint32_t slot = grid.h.prim_base + (uint32_t)kPrimEntriesPerLane * threadIdx.x;
  uint2* cells = const_cast<uint2*>(grid.cells);
  const bool ok = build_primary_list(grid, a.spheres, a.n_spheres, mk3(a.eye[0], a.eye[1], a.eye[2]), (float)row, (float)col, active,
                                     dir_at, pool_of_wave(pool).ring, cells, slot, k);
  const uint2 e0 = cells[slot], e1 = cells[slot + 1u];  // read back from the table, where bounce 0 would find them
  uint32_t* out = lists + (size_t)lane_id * 6;
  out[0] = ok ? 1u : 0u;
  out[1] = (uint32_t)k;
  out[2] = e0.x;
  out[3] = e0.y;
  out[4] = e1.x;
  out[5] = e1.y;
}

}  // namespace pt

hipError_t pt_launch_primary_masks_dump(const PrimaryDumpArgs& a, uint32_t* masks, float* dirs) {
  const size_t lds = ((size_t)a.n_spheres * 4 + pt::kTablesF4) * sizeof(float4);
  if (a.n_spheres < 1 || a.width < 1 || !a.tile_pixels || lds > 64 * 1024) return hipErrorInvalidValue;
  const unsigned blocks = (a.tile_pixels + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS;
  hipLaunchKernelGGL(pt::primary_masks_dump_kernel, dim3(blocks), dim3(PT_BLOCK_THREADS), lds, 0, a, masks, dirs);
  return hipGetLastError();
}

hipError_t pt_launch_primary_lists_dump(const PrimaryDumpArgs& a, const uint32_t* accel, int threads, uint32_t* lists) {
  const bool wide = threads == PT_GRID_WIDE_THREADS;
  if ((threads != PT_GRID_BLOCK_THREADS && !wide) || a.n_spheres < 1 || a.n_spheres > pt::kGridMaxSpheres || a.width < 1 || !a.tile_pixels)
    return hipErrorInvalidValue;
  const size_t lds = pt::kTablesF4 * sizeof(float4) + ((pt::grid_lds_bytes(a.n_spheres, true, threads) + 15) & ~(size_t)15) +
                     (size_t)(threads / 64) * pt::kPoolWaveBytes;
  const size_t lds_budget = wide ? (size_t)PT_LDS_WIDE_BUDGET_BYTES : (size_t)PT_LDS_BUDGET_BYTES;
  if (lds > lds_budget) return hipErrorInvalidValue;
  const auto fn = wide ? pt::primary_lists_dump_kernel<PT_GRID_WIDE_THREADS> : pt::primary_lists_dump_kernel<PT_GRID_BLOCK_THREADS>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_budget);
    if (e != hipSuccess) return e;
  }
  const unsigned blocks = (a.tile_pixels + (unsigned)threads - 1) / (unsigned)threads;
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(threads), lds, 0, a, accel, lists);
  return hipGetLastError();
}
#endif  // PT_BUILD_EXPERIMENTS
