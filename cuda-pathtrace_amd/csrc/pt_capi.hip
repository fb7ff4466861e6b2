// pt_capi.hip -- the C ABI of include/ptcore.h on top of the HIP runtime.
// Host code only; device code is in pt_kernel.hip.  No CPU fallback exists: every compute
// entry point fails with PT_ENODEVICE / PT_EHIP when no gfx950 device is usable.
#include <hip/hip_runtime.h>
#include <math.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "pt_internal.h"
#include "pt_kernel.h"

namespace {
thread_local char g_err[512] = "";
}

int pt_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

struct pt_renderer {
  int width = 0, height = 0, spp = 0, threads_per_block = 0;
  pt_renderer_opts opts{};
  uint32_t tile_pixels = 0;
  uint32_t frame = 0;
  uint32_t* d_state = nullptr;  // xorwow persistent state (Renderer::d_states), or nullptr
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  int device = 0;
  int launch_variant = 0;  // what fill_args chose for the launch being prepared
  // automatic variant choice (opts.variant == PT_VARIANT_AUTO)
  bool auto_variant = false;
  uint64_t resident_pixels = 0;  // one-lane-per-pixel lanes the device holds at four waves per SIMD
  double waves_per_simd = 1e9;   // one-lane-per-pixel waves of the tile per SIMD
  bool small_tile = false;       // fewer than three one-lane-per-pixel waves per SIMD (many-sphere scenes: four lanes per pixel pay there)
  bool spec_ok = true;           // variant 8's speculation has not been failing on this scene
  uint32_t* d_fail = nullptr;    // device counter written by variant 8
  uint32_t* h_fail = nullptr;    // pinned host copy, valid once ev_fail has completed
  hipEvent_t ev_fail = nullptr;
  bool fail_pending = false;
  uint32_t* d_accel = nullptr;   // variant 11's grid tables (rebuilt on the device before every frame)
  uint32_t* d_chunk = nullptr;   // sample chunking (pt_kernel.hip): PT_CHUNK_WORDS words per tile pixel + one flag per pixel block; allocated
                                 // by the first launch that chunks (never for renderers whose kernels do not), or null
  // how many chunks a frame of this renderer is split into when the kernel supports it (0 = off), per chunk family of the
  // variant table: variant 6, the split kernels (variants 8, 9), the pooled grid kernel (variant 13)
  uint32_t chunks[PT_CHUNK_FAMILIES] = {};
  uint64_t chunk_wait_ticks = 0;  // how long a chunk waits for its predecessor (wall-clock ticks of the device)
  long chunk_wait_ms = 0;         // ... the same in milliseconds (env PT_CHUNK_TIMEOUT_MS, default 4000)
  uint32_t repaired = 0;          // frames whose broken chunk chain pt_renderer_render repaired (pt_renderer_check reports it)
  float* d_vertices = nullptr;    // pt_renderer_set_display: the display vertices every frame also writes, or null
  uint32_t* d_err = nullptr;      // device error word (PT_DEVERR_*), raised by a kernel that could not go on correctly
  uint32_t* h_err = nullptr;      // pinned host copy, valid once ev_err has completed
  hipEvent_t ev_err = nullptr;
  bool err_pending = false;       // a chunked launch's error word is on its way to h_err
  uint32_t debug = 0;             // PT_DEBUG_* (lab library only, env PT_LAB_DEBUG)
  uint32_t batch_launches = 0;    // successful pt_launch_frames_kernel calls (the lab library reports it: pt_debug_renderer_batch_launches)
  // The renderer owns single-instance device scratch (generator state, d_accel, d_fail): launches of one
  // renderer must execute in submission order even when the caller alternates streams.
  hipEvent_t ev_last = nullptr;   // recorded after every launch on the stream it went to
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  // sphere materials (pt_renderer_set_materials, pt_materials.hip): while d_materials is set every launch is the materials kernel's
  void* d_materials = nullptr;    // one 16-byte row per sphere
  int n_materials = 0;
  // direct light sampling (pt_renderer_set_light_sampling): every launch is the materials kernel's LIGHTS build, on d_materials
  // or, without a table, on d_all_diffuse (PT_MATERIALS_MAX_SPHERES zeroed rows: kind DIFFUSE, param 0)
  bool light_sampling = false;
  void* d_all_diffuse = nullptr;
  // sky and sun (pt_renderer_set_sky): every launch is a SKY build of the materials kernel, on d_materials or d_all_diffuse
  bool has_sky = false;
  PtSkyConsts sky = {};
};

// the kernels outside the variant table (pt_fast.hip, pt_materials.hip): no row to read, no chunking, no frame batches
static bool lights_variant(int variant) { return variant == PT_VARIANT_MATERIALS_LIGHTS || variant == PT_VARIANT_MATERIALS_LIGHTS_SKY; }
static bool sky_variant(int variant) { return variant == PT_VARIANT_MATERIALS_SKY || variant == PT_VARIANT_MATERIALS_LIGHTS_SKY; }
static bool materials_variant(int variant) { return variant == PT_VARIANT_MATERIALS || lights_variant(variant) || sky_variant(variant); }
static bool outside_table(int variant) { return variant == PT_VARIANT_FAST || materials_variant(variant); }

// the chunk count of the variant's chunk family (0: the variant belongs to none)
static uint32_t chunks_of(const pt_renderer* r, int variant) {
  const int family = pt_kernel_variant(variant).chunk_family;
  return family == PT_CHUNK_NONE ? 0u : r->chunks[family];
}
static void chunks_off(pt_renderer* r) {
  for (uint32_t& c : r->chunks) c = 0u;
}

// the numbers of the variants whose property `has` is `want`, as "0, 6, 8": the lists in messages follow the variant table
static const char* variant_list(char (&buf)[64], bool VariantInfo::*has, bool want = true) {
  buf[0] = 0;
  for (int v = 0, at = 0; v < pt_kernel_num_variants(); v++)
    if (pt_kernel_variant(v).*has == want) at += snprintf(buf + at, sizeof(buf) - (size_t)at, at ? ", %d" : "%d", v);
  return buf;
}

// Order this launch after the renderer's previous one if that went to a different stream.
static int order_after_last(pt_renderer* r, hipStream_t stream) {
  if (r->have_last && r->last_stream != stream) PT_HIP(hipStreamWaitEvent(stream, r->ev_last, 0));
  return PT_OK;
}

static int mark_last(pt_renderer* r, hipStream_t stream) {
  PT_HIP(hipEventRecord(r->ev_last, stream));
  r->last_stream = stream;
  r->have_last = true;
  return PT_OK;
}

// ---- which kernel for a small scene: a cost model instead of a table of bands (round 4) ---------------------------------
// Three kernels render the reference's scene bit-identically: variant 6 (one lane per pixel), 9 (two) and 8 (four).  More lanes
// per pixel = more, shorter waves: they fill a tile that gives each SIMD only a wave or two, and they pay for it with the
// generator skip-ahead and the record exchange.  Per kernel, three measured constants describe a SIMD that holds k of its
// waves (ms per 1024 samples of 5 bounces): L, what one wave needs alone (latency-bound), I, what each wave adds once the SIMD
// is issue-bound -- time(k) = (L^4 + (k I)^4)^(1/4), the smooth maximum of the two regimes -- and the round size, the waves a
// SIMD works on at a time when the frame is too short for sample chunking (then the tile is whole rounds plus a rest; a
// chunked frame fills its tail and behaves as one round of any size).  Unchunked waves run `unchunked` times slower (their
// tail is not filled) and every wave costs `per_wave` of prologue.  The tile has w one-lane waves per SIMD, hence
// ceil(lanes * w) waves of the kernel in question.  Fitted to profiles/r04/tile_policy_sweep.txt (row tiles of the headline
// frame, 1024 spp, both generators: the model's choice is within 0.5 % of the measured optimum at every point) and
// profiles/r04/short_frames_*.txt (256^2 ... 640^2 at 4 ... 256 spp: within 2.3 %); tests/test_policy_model.py keeps it so.
struct KernelCost {
  int variant, lanes;
  double L, I;
  int round;
  double unchunked, per_wave;
};
static const KernelCost kKernelCost[2][3] = {
    // cuRAND XORWOW (the split kernels re-generate their partners' draws)
    {{6, 1, 6.58, 2.97, 5, 1.031, 0.00666}, {8, 4, 1.85, 0.868, 5, 1.076, 0.00248}, {9, 2, 3.40, 1.60, 8, 1.108, 0.00448}},
    // Philox (counter-based: no skip-ahead)
    {{6, 1, 6.67, 3.05, 5, 1.031, 0.00666}, {8, 4, 1.75, 0.810, 8, 1.076, 0.00248}, {9, 2, 3.35, 1.60, 8, 1.108, 0.00448}}};
static const double kLaunchMs = 0.012;

static double predicted_ms(const KernelCost& c, double w, int spp, int bounces, bool chunked) {
  auto simd = [&](double k) { return c.I > 0 ? pow(pow(c.L, 4) + pow(k * c.I, 4), 0.25) : 0.0; };
  const double k = ceil(c.lanes * w - 1e-9), u = chunked ? 1.0 : c.unchunked;
  double t = simd(k);
  if (!chunked && k > c.round) {
    const double full = floor(k / c.round), rest = k - full * c.round;
    t = full * simd(c.round) + (rest > 0 ? simd(rest) : 0.0);
  }
  return kLaunchMs + k * c.per_wave + u * t * spp / 1024.0 * bounces / 5.0;
}

// the cheapest of variants 6, 8 (and 9 where it has a build: the reference configuration) for this tile
// chunked_mask: bit v set = a launch of variant v would chunk its samples (the regime is a property of the renderer --
// opts.chunks, PT_CHUNKS, a failed hand-over allocation, a broken chain all switch chunking off -- not of spp alone)
static int cheapest_variant(int rng_mode, double w, int spp, int bounces, bool with9, uint32_t chunked_mask) {
  int best = PT_DEFAULT_VARIANT;
  double best_ms = 1e300;
  for (const KernelCost& c : kKernelCost[rng_mode == PT_RNG_PHILOX ? 1 : 0]) {
    if (c.variant == 9 && !with9) continue;
    const double ms = predicted_ms(c, w, spp, bounces, ((chunked_mask >> c.variant) & 1u) != 0u);
    if (ms < best_ms) best = c.variant, best_ms = ms;  // (variant 6 comes first: it keeps a tie)
  }
  return best;
}

static int effective_variant(pt_renderer* r, int n_spheres) {
  if (r->opts.fast_math) return PT_VARIANT_FAST;
  if (r->has_sky) return r->light_sampling ? PT_VARIANT_MATERIALS_LIGHTS_SKY : PT_VARIANT_MATERIALS_SKY;  // (pt_renderer_set_sky: as below)
  if (r->light_sampling) return PT_VARIANT_MATERIALS_LIGHTS;  // (never with fast_math or an explicit variant either)
  if (r->d_materials) return PT_VARIANT_MATERIALS;  // (never with fast_math or an explicit variant: pt_renderer_set_materials)
  if (!r->auto_variant) return r->opts.variant;
  if (r->fail_pending && hipEventQuery(r->ev_fail) == hipSuccess) {
    r->fail_pending = false;
    if (*r->h_fail > r->tile_pixels / 50u) r->spec_ok = false;  // > 2 % of the pixels left speculative mode: an open scene
  }
  // Many-sphere scenes: a bounce is n sphere tests; what matters is WHICH spheres are tested (the uniform grid with pooled
  // tests, variant 13: 160 ... 2048 spheres, from 72 on tiles that fill the chip) and that lanes whose path left the scene do not idle (path regeneration, variant
  // 10); a small closed tile still gains from four lanes per pixel until the speculation feedback says the scene is open.
  // (above ~1200 spheres the cell table wants more LDS than half a CU's: the same kernel with 1024-thread workgroups, one per CU --
  // 1024^2 x 32 spp closed / open, variant 13 | 14: 1200 spheres 13.8 / 4.3 | 12.3 / 3.6 ms, 1500: 18.0 / 6.3 | 15.6 / 5.0,
  // 2000: 69.4 / 34.5 | 18.4 / 6.2; at 1000 spheres and 256 spp 71.1 / 22.6 | 78.7 / 25.1: profiles/r05/large_scenes.txt)
  if (n_spheres > PT_GRID_WIDE_MIN_SPHERES && n_spheres <= PT_GRID_MAX_SPHERES) return 14;
  if (n_spheres >= PT_GRID_MIN_SPHERES && n_spheres <= PT_GRID_MAX_SPHERES) return 13;
  if (n_spheres >= PT_GRID_MIN_SPHERES_LARGE_TILE && n_spheres < PT_GRID_MIN_SPHERES && !r->small_tile) return 13;
  const bool xorwow = r->opts.rng_mode == PT_RNG_XORWOW;
  if (n_spheres > PT_SCREEN_MAX_SPHERES) return (xorwow && r->small_tile && r->spec_ok && r->spp >= 8) ? 8 : 10;
  // splitting a pixel's samples over lanes needs samples to split, and (xorwow) a speculation that holds
  if (r->spp < 4 || (xorwow && !r->spec_ok)) return PT_DEFAULT_VARIANT;
  const bool planar = r->opts.layout == PT_LAYOUT_PLANAR;
  const bool ref = pt_kernel_ref_bounces(n_spheres, r->opts.max_bounces, 9, planar) != 0;
  uint32_t chunked_mask = 0u;
  for (const KernelCost& k : kKernelCost[0]) {  // (the candidates of cheapest_variant)
    const uint32_t c = chunks_of(r, k.variant);
    if (c >= 2u && pt_kernel_chunked(k.variant, n_spheres, r->opts.max_bounces, planar, r->spp, c)) chunked_mask |= 1u << k.variant;
  }
  return cheapest_variant(r->opts.rng_mode, r->waves_per_simd, r->spp, r->opts.max_bounces > 0 ? r->opts.max_bounces : 1, ref, chunked_mask);
}

// opts.chunks, or env PT_CHUNKS when that is 0: 0 = automatic, 1 = never, 2..PT_CHUNKS_MAX = that many (anything else: automatic)
static int requested_chunks(int opt) {
  int want = opt;
  if (want == 0) {
    const char* env = getenv("PT_CHUNKS");
    if (env && *env) want = atoi(env);
  }
  return (want < 0 || want > PT_CHUNKS_MAX) ? 0 : want;
}

// A chunk may be at most max_samples long (the worst chained wait must stay far inside the wait limit): more chunks for very
// long frames, none at all if even PT_CHUNKS_MAX are not enough.  Returns the chunk count to use, 0 = no chunking.
static uint32_t fit_chunks(int want, int spp, int max_samples) {
  while (want >= 2 && want < PT_CHUNKS_MAX && (spp + want - 1) / want > max_samples) want *= 2;
  if (want < 2 || want > PT_CHUNKS_MAX || (spp + want - 1) / want > max_samples) return 0u;
  return (uint32_t)want;
}

// The chunk counts of a new renderer, one per chunk family.
// Sample chunking pays on frames that make few rounds of long workgroups (tools/shape_sweep.py): at least 512 samples per
// pixel and at most 8 one-lane waves per SIMD slot-round.  opts.chunks / env PT_CHUNKS: 0 = this policy, 1 = never, n = n chunks.
// The hand-over buffer (104 B per tile pixel) is allocated by the first launch that really chunks (chunk_buffer()).
static void set_chunk_counts(pt_renderer* r, const hipDeviceProp_t& prop) {
  // opts.chunks / env PT_CHUNKS, one reading for all three kernel families: 0 = the policies below, 1 = never, n = n chunks
  const int asked = requested_chunks(r->opts.chunks);
  int want = asked;
  if (want == 0 && r->spp >= 512 && r->tile_pixels > 0) {
    const uint64_t slots = (uint64_t)prop.multiProcessorCount * 4u * 4u * 64u;  // pixels resident at 4 waves per SIMD
    // The whole frame: two chunks (one hand-over per pixel; 49.95 -> 49.48 ms, eight: 49.40).  Row tiles -- what a rank of a multi-GPU
    // run renders -- are one or two rounds of waves and gain more from more chunks (tools/chunk_tile.py, profiles/r03/README.md;
    // chunks 1 / 2 / 4 / 6 / 8): 1/4 frame 13.03 / 13.31 / 12.71 / 13.03 / 12.62 ms, 1/2 frame 25.50 / 25.28 / 25.39 / 25.58 / 24.89,
    // 3/16 frame 10.31 / 10.05 / 10.15 / 9.81 / 10.61 (the steps: chunks x waves per SIMD against the five resident).
    if ((uint64_t)r->tile_pixels <= 8u * slots)
      want = r->waves_per_simd > 8.5 ? PT_CHUNKS : (r->waves_per_simd > 3.25 ? PT_CHUNKS_TILE : PT_CHUNKS_SMALL_TILE);
  }
  r->chunks[PT_CHUNK_ONE_LANE] = fit_chunks(want, r->spp, PT_CHUNK_MAX_SAMPLES);
  // The pooled grid kernel (variant 13): 512-pixel workgroups, two resident per CU, 25 ms each at 1000 spheres x 256 spp --
  // a 1024^2 frame is FOUR rounds of them and its time is whatever the last round's stragglers make it (measured: 98 or 107 ms
  // from one frame to the next, profiles/r03/README.md).  Enough chunks for about thirty-two rounds, each at least 32 samples
  // long (closed / open at 256 spp, chunks 1: 98-109 / 38.4 ms, 2: 101.5 / 36.4, 4: 97.3 / 35.4, 8: 96.0 / 35.1, 16: 97.9 / 36.3).
  // Its samples are a hundred times as long as the nine-sphere kernel's (about 0.1 ms per sample and workgroup at 1000
  // spheres), so a chunk is capped at PT_CHUNK_MAX_SAMPLES_GRID samples: the worst chained wait -- all chunks of a block
  // co-resident, chunk k waits k chunk durations -- stays a fraction of a second.
  int want13 = asked;
  if (want13 == 0 && r->tile_pixels > 0) {
    const uint64_t resident = (uint64_t)prop.multiProcessorCount * 2u;  // workgroups
    const uint64_t groups = ((uint64_t)r->tile_pixels + 511u) / 512u;
    const uint64_t rounds = (groups + resident - 1) / resident;
    want13 = rounds >= 32 ? 1 : (int)((32 + rounds - 1) / rounds);
    if (want13 > PT_CHUNKS_GRID_MAX) want13 = PT_CHUNKS_GRID_MAX;
    while (want13 >= 2 && r->spp / want13 < 32) want13 /= 2;
    // Round 5: a tile whose workgroups fill at most HALF the chip's slots gains nothing from chunk workgroups -- they are resident
    // at once and only wait for their predecessors, in slots the working ones could have had to themselves (rows 512..640 of
    // the 1000-sphere frame, closed / open: 8 chunks 29.1 / 19.1 ms, none 17.9 / 10.4; profiles/r05/cfg4_tile_chunks.txt)
    if (groups * 2u <= resident) want13 = 1;
  }
  r->chunks[PT_CHUNK_GRID] = fit_chunks(want13, r->spp, PT_CHUNK_MAX_SAMPLES_GRID);
  // the split kernels (small tiles of the reference configuration: one or two rounds of waves by construction): four chunks
  // (tools/chunk_tile.py, profiles/r03/tile_policy_bitops.txt)
  r->chunks[PT_CHUNK_SPLIT] = fit_chunks(asked == 0 && r->spp >= 512 ? PT_CHUNKS_SPLIT : asked, r->spp, PT_CHUNK_MAX_SAMPLES);
}

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }
#ifndef PT_BUILD_FINGERPRINT
#define PT_BUILD_FINGERPRINT "unknown"
#endif
const char* pt_build_fingerprint(void) { return PT_BUILD_FINGERPRINT; }
const char* pt_last_error(void) { return g_err; }

int pt_set_device(int device) {
  PT_HIP(hipSetDevice(device));
  return PT_OK;
}

int pt_device_count(int* count) {
  if (!count) return pt_fail(PT_EINVAL, "pt_device_count: count is NULL");
  *count = 0;
  PT_HIP(hipGetDeviceCount(count));
  return PT_OK;
}

int pt_device_info(char* name, size_t name_len, int* compute_units, int* clock_khz) {
  int dev = 0;
  PT_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  PT_HIP(hipGetDeviceProperties(&prop, dev));
  if (name && name_len) snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (clock_khz) *clock_khz = prop.clockRate;
  return PT_OK;
}

int pt_malloc(void** d_ptr, size_t bytes) {
  if (!d_ptr) return pt_fail(PT_EINVAL, "pt_malloc: d_ptr is NULL");
  PT_HIP(hipMalloc(d_ptr, bytes));
  return PT_OK;
}

int pt_free(void* d_ptr) {
  PT_HIP(hipFree(d_ptr));
  return PT_OK;
}

int pt_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
  PT_HIP(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return PT_OK;
}

int pt_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
  PT_HIP(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_memset(void* d_ptr, int value, size_t bytes) {
  PT_HIP(hipMemset(d_ptr, value, bytes));
  return PT_OK;
}

int pt_device_synchronize(void) {
  PT_HIP(hipDeviceSynchronize());
  return PT_OK;
}

void pt_renderer_opts_default(pt_renderer_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->max_bounces = 5;
  o->rng_mode = PT_RNG_XORWOW;
  o->persist_rng = 1;
  o->variant = PT_VARIANT_AUTO;
  o->layout = PT_LAYOUT_INTERLEAVED;
  o->fast_math = 0;
  o->chunks = 0;
}

static int setup_random(pt_renderer* r) {
  if (!r->d_state) return PT_OK;
  PT_HIP(pt_launch_setup_random(r->d_state, r->width, r->opts.row_begin, r->tile_pixels, r->opts.seed, nullptr));
  // The reference launches setup_random unchecked and unsynchronised (Renderer.h:38) because its
  // only stream orders the next launch after it.  pt_renderer_enqueue may run on ANY caller stream
  // (possibly non-blocking with respect to the default stream), so finish the 10 us kernel here.
  PT_HIP(hipStreamSynchronize(nullptr));
  return PT_OK;
}

int pt_renderer_create(int width, int height, int samples_per_pixel, int threads_per_block,
                       const pt_renderer_opts* opts, pt_renderer** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_renderer_create: out is NULL");
  *out = nullptr;
  pt_renderer_opts o;
  if (opts) o = *opts; else pt_renderer_opts_default(&o);
  if (o.row_begin == 0 && o.row_end == 0) o.row_end = height;
  if (width <= 0 || height <= 0 || samples_per_pixel <= 0)
    return pt_fail(PT_EINVAL, "pt_renderer_create: width/height/samples must be positive (%d x %d x %d)", width, height,
                   samples_per_pixel);
  if (o.row_begin < 0 || o.row_end > height || o.row_begin > o.row_end)
    return pt_fail(PT_EINVAL, "pt_renderer_create: bad row range [%d,%d) for height %d", o.row_begin, o.row_end, height);
  if (o.max_bounces < 0 || o.max_bounces > 64) return pt_fail(PT_EINVAL, "pt_renderer_create: max_bounces %d", o.max_bounces);
  if (o.rng_mode != PT_RNG_XORWOW && o.rng_mode != PT_RNG_PHILOX)
    return pt_fail(PT_EINVAL, "pt_renderer_create: rng_mode %d", o.rng_mode);
  if (o.layout != PT_LAYOUT_INTERLEAVED && o.layout != PT_LAYOUT_PLANAR) return pt_fail(PT_EINVAL, "pt_renderer_create: layout %d", o.layout);
  if (o.fast_math != 0 && o.fast_math != 1) return pt_fail(PT_EINVAL, "pt_renderer_create: fast_math %d", o.fast_math);
  if (o.fast_math && o.variant != PT_VARIANT_AUTO)
    return pt_fail(PT_EINVAL, "pt_renderer_create: fast_math has one kernel; leave variant at -1");
  if (o.chunks < 0 || o.chunks > PT_CHUNKS_MAX || o.reserved != 0)
    return pt_fail(PT_EINVAL, "pt_renderer_create: chunks %d (0 = automatic, 1 = off, 2..%d), reserved %d (must be 0)", o.chunks, PT_CHUNKS_MAX, o.reserved);
  if (o.variant != PT_VARIANT_AUTO && !pt_kernel_has_variant(o.variant)) {
    char product[64], lab[64];
    return pt_fail(PT_EINVAL, "pt_renderer_create: kernel variant %d is not in this build (product variants: %s; the experiments %s live in libptcore_lab.so)",
                   o.variant, variant_list(product, &VariantInfo::product), variant_list(lab, &VariantInfo::product, false));
  }
  // 32-bit pixel ids like the reference (pathtrace.cu:206): width*height must fit uint32
  if ((uint64_t)width * (uint64_t)height > 0xFFFFFFFFull) return pt_fail(PT_EINVAL, "pt_renderer_create: image too large");

  int ndev = 0;
  PT_HIP(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return pt_fail(PT_ENODEVICE, "pt_renderer_create: no HIP device");

  pt_renderer* r = new (std::nothrow) pt_renderer();
  if (!r) return pt_fail(PT_ENOMEM, "pt_renderer_create: out of host memory");
  r->width = width;
  r->height = height;
  r->spp = samples_per_pixel;
  r->threads_per_block = threads_per_block;
  r->opts = o;
  r->tile_pixels = (uint32_t)(o.row_end - o.row_begin) * (uint32_t)width;
  r->auto_variant = (o.variant == PT_VARIANT_AUTO);
  hipError_t e = hipGetDevice(&r->device);
  hipDeviceProp_t prop;
  if (e == hipSuccess) {
    e = hipGetDeviceProperties(&prop, r->device);
    if (e == hipSuccess) {
      const uint64_t simds = (uint64_t)prop.multiProcessorCount * 4u;
      r->resident_pixels = simds * 4u * 64u;
      r->waves_per_simd = (double)r->tile_pixels / (double)(simds * 64u);
      r->small_tile = (uint64_t)r->tile_pixels < simds * 64u * 3u;
    }
  }
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_fail, sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(r->d_fail, 0, sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc((void**)&r->h_fail, sizeof(uint32_t), hipHostMallocDefault);
  if (e == hipSuccess) { *r->h_fail = 0; e = hipEventCreateWithFlags(&r->ev_fail, hipEventDisableTiming); }
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_accel, pt_kernel_accel_bytes());
  if (e == hipSuccess) {
    set_chunk_counts(r, prop);
    int khz = 0;  // s_memrealtime ticks per millisecond
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, r->device) != hipSuccess || khz <= 0) khz = 100000;
    long wait_ms = 4000;
    if (const char* env = getenv("PT_CHUNK_TIMEOUT_MS")) { if (*env) wait_ms = atol(env); }
    if (wait_ms < 1) wait_ms = 1;
    r->chunk_wait_ticks = (uint64_t)khz * (uint64_t)wait_ms;
    r->chunk_wait_ms = wait_ms;
#if PT_BUILD_EXPERIMENTS
    if (const char* env = getenv("PT_LAB_DEBUG")) r->debug = (uint32_t)strtoul(env, nullptr, 0);
#endif
  }
  if (e == hipSuccess) e = hipMalloc((void**)&r->d_err, sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(r->d_err, 0, sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc((void**)&r->h_err, sizeof(uint32_t), hipHostMallocDefault);
  if (e == hipSuccess) { *r->h_err = 0; e = hipEventCreateWithFlags(&r->ev_err, hipEventDisableTiming); }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_last, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreate(&r->ev_start);
  if (e == hipSuccess) e = hipEventCreate(&r->ev_stop);
  if (e == hipSuccess && o.rng_mode == PT_RNG_XORWOW && o.persist_rng && r->tile_pixels)
    e = hipMalloc((void**)&r->d_state, (size_t)r->tile_pixels * 6 * sizeof(uint32_t));  // Renderer.h:37
  if (e != hipSuccess) {
    int rc = pt_fail(PT_EHIP, "pt_renderer_create: %s", hipGetErrorString(e));
    pt_renderer_destroy(r);
    return rc;
  }
  int rc = setup_random(r);  // Renderer.h:38
  if (rc != PT_OK) {
    pt_renderer_destroy(r);
    return rc;
  }
  *out = r;
  return PT_OK;
}

int pt_renderer_destroy(pt_renderer* r) {
  if (!r) return PT_OK;
  if (r->d_state) (void)hipFree(r->d_state);  // Renderer.h:50
  if (r->d_materials) (void)hipFree(r->d_materials);
  if (r->d_all_diffuse) (void)hipFree(r->d_all_diffuse);
  if (r->d_accel) (void)hipFree(r->d_accel);
  if (r->d_chunk) (void)hipFree(r->d_chunk);
  if (r->d_err) (void)hipFree(r->d_err);
  if (r->h_err) (void)hipHostFree(r->h_err);
  if (r->ev_err) (void)hipEventDestroy(r->ev_err);
  if (r->d_fail) (void)hipFree(r->d_fail);
  if (r->h_fail) (void)hipHostFree(r->h_fail);
  if (r->ev_fail) (void)hipEventDestroy(r->ev_fail);
  if (r->ev_last) (void)hipEventDestroy(r->ev_last);
  if (r->ev_start) (void)hipEventDestroy(r->ev_start);
  if (r->ev_stop) (void)hipEventDestroy(r->ev_stop);
  delete r;
  return PT_OK;
}

// Does a launch of this renderer with this variant and scene chain a pixel's samples through several workgroups?  Allocates the
// hand-over buffer the first time the answer is yes; an allocation failure turns chunking off for good (it is a scheduling
// aid, never a reason for a renderer not to work).
static bool chunk_buffer(pt_renderer* r, int variant, int n_spheres) {
  const uint32_t chunks = chunks_of(r, variant);
  if (chunks < 2u || !pt_kernel_chunked(variant, n_spheres, r->opts.max_bounces, r->opts.layout == PT_LAYOUT_PLANAR, r->spp, chunks))
    return false;
  if (r->d_chunk) return true;
  const size_t blocks = ((size_t)r->tile_pixels * 4 + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS;  // (the four-lane kernel has the most pixel blocks)
  if (hipMalloc((void**)&r->d_chunk, ((size_t)PT_CHUNK_WORDS * r->tile_pixels + blocks) * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();  // not sticky: the launch that follows must not inherit it
    r->d_chunk = nullptr;
    chunks_off(r);
    return false;
  }
  return true;
}

// The error word of an earlier chunked launch, once it has arrived (wait: block until it has).  *err receives the word (0 = the
// chain held) and is cleared on the device; a broken chain also switches chunking off for this renderer for good -- whatever
// broke it may do so again.
static int take_device_error(pt_renderer* r, bool wait, uint32_t* err) {
  *err = 0u;
  if (!r->err_pending) return PT_OK;
  if (wait) PT_HIP(hipEventSynchronize(r->ev_err));
  else if (hipEventQuery(r->ev_err) != hipSuccess) { (void)hipGetLastError(); return PT_OK; }
  r->err_pending = false;
  *err = *r->h_err;
  if (*err == 0u) return PT_OK;
  *r->h_err = 0u;
  PT_HIP(hipMemset(r->d_err, 0, sizeof(uint32_t)));
  chunks_off(r);
  return PT_OK;
}

// ... as a status: PT_EKERNEL for a frame that was enqueued and is incomplete (pt_renderer_render repairs its own instead)
static int check_device_error(pt_renderer* r, bool wait) {
  uint32_t err = 0u;
  const int rc = take_device_error(r, wait, &err);
  if (rc != PT_OK || err == 0u) return rc;
  return pt_fail(PT_EKERNEL, "render: sample-chunk chain broken (device error word 0x%x): a workgroup waited %ld ms for its "
                             "predecessor in vain; that frame is incomplete (the pixel blocks concerned were left untouched, their "
                             "generator state included), chunking is now off for this renderer", err, r->chunk_wait_ms);
}

static int fill_args(pt_renderer* r, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                     const float eye[3], PixelKernelArgs* a) {
  if (!r) return pt_fail(PT_EINVAL, "render: renderer is NULL");
  if (!d_out && r->tile_pixels) return pt_fail(PT_EINVAL, "render: d_out is NULL");
  if (n_spheres < 0 || (n_spheres > 0 && !d_spheres)) return pt_fail(PT_EINVAL, "render: bad scene (%d spheres)", n_spheres);
  if (!basis || !eye) return pt_fail(PT_EINVAL, "render: basis/eye is NULL");
  const int variant = effective_variant(r, n_spheres);
  if (materials_variant(variant) && r->d_materials && n_spheres != r->n_materials)
    return pt_fail(PT_EINVAL, "render: n_spheres %d differs from the %d entries of the material table (pt_renderer_set_materials)", n_spheres, r->n_materials);
  if (variant == PT_VARIANT_MATERIALS_LIGHTS && !r->d_materials && n_spheres > PT_MATERIALS_MAX_SPHERES)
    return pt_fail(PT_ELIMIT, "render: %d spheres exceed the %d spheres (PT_MATERIALS_MAX_SPHERES) the light-sampling kernel stages (pt_renderer_set_light_sampling)",
                   n_spheres, PT_MATERIALS_MAX_SPHERES);
  if (sky_variant(variant) && !r->d_materials && n_spheres > PT_MATERIALS_MAX_SPHERES)
    return pt_fail(PT_ELIMIT, "render: %d spheres exceed the %d spheres (PT_MATERIALS_MAX_SPHERES) the sky kernel stages (pt_renderer_set_sky)",
                   n_spheres, PT_MATERIALS_MAX_SPHERES);
  if (!outside_table(variant) && n_spheres > pt_kernel_max_spheres(variant))
    return pt_fail(PT_ELIMIT, "render: %d spheres exceed the LDS staging limit of %d", n_spheres,
                   pt_kernel_max_spheres(variant));
  a->fail_count = r->d_fail;
  a->accel = r->d_accel;
  a->scene_lds_f4 = 0;
  a->planar = r->opts.layout == PT_LAYOUT_PLANAR ? 1u : 0u;
  r->launch_variant = variant;
  a->out = d_out;
  a->spheres = d_spheres;
  a->rng_state = r->d_state;
  memcpy(a->basis, basis, sizeof(a->basis));
  memcpy(a->eye, eye, sizeof(a->eye));
  a->n_spheres = n_spheres;
  a->width = r->width;
  a->height = r->height;
  a->row_begin = r->opts.row_begin;
  a->tile_pixels = r->tile_pixels;
  a->spp = r->spp;
  a->max_bounces = r->opts.max_bounces;
  a->frame = r->frame;
  a->seed = r->opts.seed;
  // sample chunking: only for the kernels that chunk (reference configuration, variant 6), and only with a hand-over buffer
  const bool chunking = !outside_table(variant) && chunk_buffer(r, variant, n_spheres);
  a->chunks = chunking ? chunks_of(r, variant) : 0u;
  a->chunk_state = chunking ? r->d_chunk : nullptr;
  a->chunk_flag = chunking ? r->d_chunk + (size_t)PT_CHUNK_WORDS * r->tile_pixels : nullptr;
  // a frame that fits the chip in at most two rounds of workgroups is mostly tail: its waves set their priority by progress
  a->prio = (r->spp >= 4 && (uint64_t)r->tile_pixels <= 2u * r->resident_pixels) ? 1u : 0u;
  a->err_word = r->d_err;
  a->chunk_wait_ticks = r->chunk_wait_ticks;
  a->debug = r->debug;
  a->repair = 0u;
  a->vertices = r->d_vertices;
  return PT_OK;
}

// With the automatic policy a speculative launch is bracketed by the reset and the asynchronous
// read-back of its failure counter (consulted by a later effective_variant()).  The bracket sits
// OUTSIDE the event pair of pt_renderer_render so the returned kernel time is not distorted.
static hipError_t launch(pt_renderer* r, const PixelKernelArgs& a, hipStream_t stream) {
  if (r->launch_variant == PT_VARIANT_FAST) return pt_launch_fast_kernel(a, r->opts.rng_mode, stream);
  if (r->launch_variant == PT_VARIANT_MATERIALS) return pt_launch_materials_kernel(a, r->d_materials, r->opts.rng_mode, false, nullptr, stream);
  if (materials_variant(r->launch_variant))
    return pt_launch_materials_kernel(a, r->d_materials ? r->d_materials : r->d_all_diffuse, r->opts.rng_mode, lights_variant(r->launch_variant),
                                      sky_variant(r->launch_variant) ? &r->sky : nullptr, stream);
  return pt_launch_pixel_kernel(a, r->opts.rng_mode, r->launch_variant, stream);
}

static int watch_begin(pt_renderer* r, hipStream_t stream, bool* watching) {
  *watching = r->auto_variant && pt_kernel_variant(r->launch_variant).split() && !r->fail_pending;
  if (*watching) PT_HIP(hipMemsetAsync(r->d_fail, 0, sizeof(uint32_t), stream));
  return PT_OK;
}

static int watch_error(pt_renderer* r, const PixelKernelArgs& a, hipStream_t stream) {
  if (a.chunks < 2u) return PT_OK;  // only chunked launches can raise the word
  PT_HIP(hipMemcpyAsync(r->h_err, r->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  PT_HIP(hipEventRecord(r->ev_err, stream));
  r->err_pending = true;
  return PT_OK;
}

static int watch_end(pt_renderer* r, hipStream_t stream, bool watching) {
  if (!watching) return PT_OK;
  PT_HIP(hipMemcpyAsync(r->h_fail, r->d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  PT_HIP(hipEventRecord(r->ev_fail, stream));
  r->fail_pending = true;
  return PT_OK;
}

int pt_renderer_enqueue(pt_renderer* r, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                        const float eye[3], void* hip_stream) {
  PixelKernelArgs a;
  if (!r) return pt_fail(PT_EINVAL, "render: renderer is NULL");
  int rc = check_device_error(r, false);  // an earlier asynchronous frame whose chain broke is reported here
  if (rc != PT_OK) return rc;
  rc = fill_args(r, d_out, d_spheres, n_spheres, basis, eye, &a);
  if (rc != PT_OK) return rc;
  if (r->tile_pixels == 0) return PT_OK;
  rc = order_after_last(r, (hipStream_t)hip_stream);
  if (rc != PT_OK) return rc;
  bool watching = false;
  rc = watch_begin(r, (hipStream_t)hip_stream, &watching);
  if (rc != PT_OK) return rc;
  PT_HIP(launch(r, a, (hipStream_t)hip_stream));
  rc = watch_end(r, (hipStream_t)hip_stream, watching);
  if (rc != PT_OK) return rc;
  rc = watch_error(r, a, (hipStream_t)hip_stream);
  if (rc != PT_OK) return rc;
  rc = mark_last(r, (hipStream_t)hip_stream);
  if (rc != PT_OK) return rc;
  r->frame++;
  return PT_OK;
}

// A batch of frames with known cameras (include/ptcore.h).  Where a frames kernel exists -- the reference's scene in the
// reference configuration, i.e. the interactive shape -- the batch goes out as launches of up to PT_FRAMES_MAX frames each;
// everywhere else, and whenever two frames would share a buffer, it is the loop of single-frame enqueues it stands for.
// So is the batch of an XORWOW renderer that does not persist its state: each of its single frames starts from the seeded
// stream (pixel_kernel, xorwow_init), while the frames kernel seeds once and keeps the generator in registers across its frames.
// (The counter-based generator's key depends only on the frame counter: batched with or without persist_rng.)
int pt_renderer_enqueue_frames(pt_renderer* r, int n_frames, float* d_out, size_t out_stride_floats, float* d_vertices,
                               size_t vtx_stride_floats, const pt_sphere* d_spheres, int n_spheres, const float* bases,
                               const float* eyes, void* hip_stream) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_enqueue_frames: renderer is NULL");
  if (n_frames < 0 || (n_frames > 0 && (!bases || !eyes))) return pt_fail(PT_EINVAL, "pt_renderer_enqueue_frames: bad arguments");
  if (r->light_sampling)
    return pt_fail(PT_EINVAL, "pt_renderer_enqueue_frames: the renderer samples its lights directly (pt_renderer_set_light_sampling); the light-sampling kernel has no frame batches");
  if (n_frames == 0) return PT_OK;
  float* const saved_vertices = r->d_vertices;
  const size_t tile_floats = (size_t)r->tile_pixels * 14u, vtx_floats = (size_t)r->tile_pixels * 3u;
  const int variant = effective_variant(r, n_spheres);
  const bool batched = n_frames >= 2 && r->tile_pixels > 0 && !outside_table(variant) &&
                       pt_kernel_has_frames(variant, n_spheres, r->opts.max_bounces, r->opts.layout == PT_LAYOUT_PLANAR) &&
                       (r->opts.rng_mode != PT_RNG_XORWOW || r->d_state != nullptr) &&
                       out_stride_floats >= tile_floats && (d_vertices ? vtx_stride_floats >= vtx_floats : saved_vertices == nullptr);
  int rc = PT_OK;
  for (int f0 = 0; f0 < n_frames && rc == PT_OK;) {
    const int m = batched ? (n_frames - f0 < PT_FRAMES_MAX ? n_frames - f0 : PT_FRAMES_MAX) : 1;
    float* out_f = d_out ? d_out + (size_t)f0 * out_stride_floats : nullptr;
    if (d_vertices) r->d_vertices = d_vertices + (size_t)f0 * vtx_stride_floats;
    if (m < 2) {
      rc = pt_renderer_enqueue(r, out_f, d_spheres, n_spheres, bases + 12 * (size_t)f0, eyes + 3 * (size_t)f0, hip_stream);
      f0 += 1;
      continue;
    }
    FramesKernelArgs fa;
    rc = check_device_error(r, false);
    if (rc != PT_OK) break;
    rc = fill_args(r, out_f, d_spheres, n_spheres, bases + 12 * (size_t)f0, eyes + 3 * (size_t)f0, &fa.base);
    if (rc != PT_OK) break;
    fa.base.chunks = 0u;  // (a batch's workgroups keep their pixel block: nothing is handed from workgroup to workgroup)
    fa.base.chunk_state = nullptr;
    fa.base.chunk_flag = nullptr;
    fa.frames = (uint32_t)m;
    fa.out_stride = out_stride_floats;
    fa.vtx_stride = vtx_stride_floats;
    for (int k = 0; k < m; k++) {
      memcpy(fa.cams[k], bases + 12 * (size_t)(f0 + k), 12 * sizeof(float));
      memcpy(fa.cams[k] + 12, eyes + 3 * (size_t)(f0 + k), 3 * sizeof(float));
    }
    rc = order_after_last(r, (hipStream_t)hip_stream);
    if (rc != PT_OK) break;
    {
      const hipError_t e = pt_launch_frames_kernel(fa, r->opts.rng_mode, variant, (hipStream_t)hip_stream);
      if (e != hipSuccess) { rc = pt_fail(PT_EHIP, "pt_renderer_enqueue_frames: %s", hipGetErrorString(e)); break; }
      r->batch_launches++;
    }
    rc = mark_last(r, (hipStream_t)hip_stream);
    r->frame += (uint32_t)m;
    f0 += m;
  }
  r->d_vertices = saved_vertices;
  return rc;
}

#if PT_BUILD_EXPERIMENTS
// lab library: how many launches of the frames kernel this renderer has made (include/ptcore_lab.h)
int pt_debug_renderer_batch_launches(pt_renderer* r, uint32_t* launches) {
  if (!r || !launches) return pt_fail(PT_EINVAL, "pt_debug_renderer_batch_launches: NULL argument");
  *launches = r->batch_launches;
  return PT_OK;
}
#endif

int pt_renderer_render(pt_renderer* r, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                       const float eye[3], float* ms_out) {
  PixelKernelArgs a;
  if (!r) return pt_fail(PT_EINVAL, "render: renderer is NULL");
  int rc = check_device_error(r, true);
  if (rc != PT_OK) return rc;
  rc = fill_args(r, d_out, d_spheres, n_spheres, basis, eye, &a);
  if (rc != PT_OK) return rc;
  if (ms_out) *ms_out = 0.0f;
  if (r->tile_pixels == 0) return PT_OK;
  rc = order_after_last(r, nullptr);
  if (rc != PT_OK) return rc;
  bool watching = false;
  rc = watch_begin(r, nullptr, &watching);
  if (rc != PT_OK) return rc;
  PT_HIP(hipEventRecord(r->ev_start, nullptr));  // Renderer.h:68
  PT_HIP(launch(r, a, nullptr));
  PT_HIP(hipEventRecord(r->ev_stop, nullptr));   // Renderer.h:70
  rc = watch_end(r, nullptr, watching);
  if (rc != PT_OK) return rc;
  rc = watch_error(r, a, nullptr);
  if (rc != PT_OK) return rc;
  PT_HIP(hipEventSynchronize(r->ev_stop));       // Renderer.h:72
  r->have_last = false;  // the launch has completed: nothing left to order against
  r->frame++;
  float ms = 0.0f;
  PT_HIP(hipEventElapsedTime(&ms, r->ev_start, r->ev_stop));
  // A synchronous frame whose chunk chain broke is completed HERE: the chunked launch left every pixel block either complete
  // or untouched, generator state included (pt_kernel.hip, chunk_wait), so one unchunked launch over the untouched blocks
  // makes the frame -- and the state the next frame starts from -- exactly what an unbroken launch would have left.
  uint32_t err = 0u;
  rc = take_device_error(r, true, &err);
  if (rc != PT_OK) return rc;
  if (err != 0u) {
    a.repair = a.chunks;  // the count a complete block's flag holds
    a.chunks = 0u;
    PT_HIP(hipEventRecord(r->ev_start, nullptr));
    PT_HIP(launch(r, a, nullptr));
    PT_HIP(hipEventRecord(r->ev_stop, nullptr));
    PT_HIP(hipEventSynchronize(r->ev_stop));
    float ms2 = 0.0f;
    PT_HIP(hipEventElapsedTime(&ms2, r->ev_start, r->ev_stop));
    ms += ms2;
    r->repaired++;
    // not an error (the frame is complete), but never silent either: the caller's frame time holds the whole wait
    snprintf(g_err, sizeof(g_err), "render: sample-chunk chain broken (device error word 0x%x) -- frame repaired in place by a second, unchunked "
             "launch over the untouched pixel blocks; the returned time includes the %ld ms wait; chunking is now off for this renderer", err, r->chunk_wait_ms);
    fprintf(stderr, "ptcore: %s\n", g_err);
  }
  if (ms_out) *ms_out = ms;
  return PT_OK;
}

int pt_renderer_check(pt_renderer* r, int wait, uint32_t* repaired_frames) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_check: renderer is NULL");
  if (repaired_frames) *repaired_frames = r->repaired;
  return check_device_error(r, wait != 0);
}

// ---- progressive sessions (include/ptcore.h: the contract; pt_kernel.hip, pixel_kernel RESUME: the passes) ------------------
// The reference's interactive loop renders a resting camera's frame again and again from fresh samples (main.cu:146-177,
// pathtrace.cu:212-256); a session adds samples to one frame instead.  Its record holds each pixel's whole state between passes.
struct pt_progressive {
  pt_renderer* r = nullptr;
  uint32_t* d_rec = nullptr;            // PT_CHUNK_WORDS words per tile pixel, [word][pixel] (pixel_kernel RESUME), or null for an empty tile
  int64_t samples = 0;                  // samples per pixel so far
  float cam[15] = {};                   // the first pass's basis and eye ...
  const pt_sphere* spheres = nullptr;   // ... and scene: later passes must bring the same
  int n_spheres = 0;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  // adaptive sampling (pt_progressive_set_adaptive, pt_adaptive.hip): off unless d_adaptive is set
  void* d_adaptive = nullptr;           // one allocation: counts, list, mask, block sums, words (AdaptiveState)
  AdaptiveState ast{};
  AdaptiveRule rule{};
  pt_adaptive_opts opts{};
  bool forced = false;                  // the next pass takes mask bit 0 as it is (lab library: pt_debug_progressive_set_active)
};

// the automatic policy's choice restricted to the kernels with a resume build: where it would pick a split kernel, variant 6
static int session_variant(pt_renderer* r, int n_spheres) {
  const int v = effective_variant(r, n_spheres);
  return pt_kernel_variant(v).split() ? PT_DEFAULT_VARIANT : v;
}

int pt_progressive_create(pt_renderer* r, pt_progressive** out) {
  if (!out) return pt_fail(PT_EINVAL, "pt_progressive_create: out is NULL");
  *out = nullptr;
  if (!r) return pt_fail(PT_EINVAL, "pt_progressive_create: renderer is NULL");
  char resume[64];
  variant_list(resume, &VariantInfo::resume);
  if (r->opts.fast_math) return pt_fail(PT_EINVAL, "pt_progressive_create: a fast_math renderer has no progressive passes (resume builds: variants %s)", resume);
  if (r->d_materials) return pt_fail(PT_EINVAL, "pt_progressive_create: the renderer has a material table (pt_renderer_set_materials); the materials kernel has no progressive passes");
  if (r->has_sky) return pt_fail(PT_EINVAL, "pt_progressive_create: the renderer has a sky (pt_renderer_set_sky); the sky kernel has no progressive passes");
  if (r->light_sampling)
    return pt_fail(PT_EINVAL, "pt_progressive_create: the renderer samples its lights directly (pt_renderer_set_light_sampling); the light-sampling kernel has no progressive passes");
  if (!r->auto_variant && !pt_kernel_has_resume(r->opts.variant))
    return pt_fail(PT_EINVAL, "pt_progressive_create: kernel variant %d has no progressive passes (resume builds: variants %s)", r->opts.variant, resume);
  pt_progressive* p = new (std::nothrow) pt_progressive();
  if (!p) return pt_fail(PT_ENOMEM, "pt_progressive_create: out of host memory");
  p->r = r;
  hipError_t e = hipSuccess;
  if (r->tile_pixels) e = hipMalloc((void**)&p->d_rec, (size_t)PT_CHUNK_WORDS * r->tile_pixels * sizeof(uint32_t));
  if (e == hipSuccess) e = hipEventCreate(&p->ev_start);
  if (e == hipSuccess) e = hipEventCreate(&p->ev_stop);
  if (e != hipSuccess) {
    const int rc = pt_fail(e == hipErrorNoDevice ? PT_ENODEVICE : PT_EHIP, "pt_progressive_create: %s", hipGetErrorString(e));
    pt_progressive_destroy(p);
    return rc;
  }
  *out = p;
  return PT_OK;
}

int pt_progressive_destroy(pt_progressive* p) {
  if (!p) return PT_OK;
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_adaptive) (void)hipFree(p->d_adaptive);
  if (p->ev_start) (void)hipEventDestroy(p->ev_start);
  if (p->ev_stop) (void)hipEventDestroy(p->ev_stop);
  delete p;
  return PT_OK;
}

int pt_progressive_reset(pt_progressive* p) {
  if (!p) return pt_fail(PT_EINVAL, "pt_progressive_reset: session is NULL");
  p->samples = 0;
  p->forced = false;  // (an adaptive session's next pass is a first pass again: every pixel active, the options kept)
  return PT_OK;
}

// waits for the session's last pass (and whatever its renderer launched before it)
static int session_sync(const pt_progressive* p) {
  if (p->r->have_last) PT_HIP(hipEventSynchronize(p->r->ev_last));
  return PT_OK;
}

int pt_progressive_samples(const pt_progressive* p, int64_t* samples) {
  if (!p || !samples) return pt_fail(PT_EINVAL, "pt_progressive_samples: NULL argument");
  *samples = p->samples;
  if (p->d_adaptive && p->samples > 0 && p->r->tile_pixels) {  // the maximum per-pixel count: the total, unless the set emptied
    int rc = session_sync(p);
    if (rc != PT_OK) return rc;
    uint32_t w = 0u;
    PT_HIP(hipMemcpy(&w, p->ast.words + 1, sizeof(w), hipMemcpyDeviceToHost));
    *samples = (int64_t)w;
  }
  return PT_OK;
}

int pt_progressive_variant(const pt_progressive* p, int n_spheres, int* variant) {
  if (!p || !variant) return pt_fail(PT_EINVAL, "pt_progressive_variant: NULL argument");
  *variant = session_variant(p->r, n_spheres);
  return PT_OK;
}

// Checks a pass and fills its arguments; *empty = the tile has no pixels (the pass only counts)
static int progressive_args(pt_progressive* p, int spp, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                            const float eye[3], ResumeKernelArgs* ra, int* variant) {
  if (!p) return pt_fail(PT_EINVAL, "pt_progressive: session is NULL");
  pt_renderer* r = p->r;
  if (spp < 1) return pt_fail(PT_EINVAL, "pt_progressive: spp %d (a pass adds at least one sample)", spp);
  if (!d_out && r->tile_pixels) return pt_fail(PT_EINVAL, "pt_progressive: d_out is NULL");
  if (n_spheres < 0 || (n_spheres > 0 && !d_spheres)) return pt_fail(PT_EINVAL, "pt_progressive: bad scene (%d spheres)", n_spheres);
  if (!basis || !eye) return pt_fail(PT_EINVAL, "pt_progressive: basis/eye is NULL");
  if ((int64_t)spp > (int64_t)INT_MAX - p->samples)
    return pt_fail(PT_EINVAL, "pt_progressive: %lld + %d samples exceed INT_MAX (the reference's counts are int)", (long long)p->samples, spp);
  if (p->samples > 0 && (memcmp(p->cam, basis, 12 * sizeof(float)) != 0 || memcmp(p->cam + 12, eye, 3 * sizeof(float)) != 0 ||
                         p->spheres != d_spheres || p->n_spheres != n_spheres))
    return pt_fail(PT_EINVAL, "pt_progressive: camera or scene differs from the session's first pass: reset the session");
  if (r->d_materials) return pt_fail(PT_EINVAL, "pt_progressive: the renderer has a material table (pt_renderer_set_materials); the materials kernel has no progressive passes");
  if (r->has_sky) return pt_fail(PT_EINVAL, "pt_progressive: the renderer has a sky (pt_renderer_set_sky); the sky kernel has no progressive passes");
  if (r->light_sampling)
    return pt_fail(PT_EINVAL, "pt_progressive: the renderer samples its lights directly (pt_renderer_set_light_sampling); the light-sampling kernel has no progressive passes");
  const int v = session_variant(r, n_spheres);
  if (!pt_kernel_has_resume(v)) return pt_fail(PT_EINVAL, "pt_progressive: kernel variant %d has no progressive passes", v);
  if (n_spheres > pt_kernel_max_spheres(v))
    return pt_fail(PT_ELIMIT, "pt_progressive: %d spheres exceed the LDS staging limit of %d", n_spheres, pt_kernel_max_spheres(v));
  *variant = v;
  PixelKernelArgs& a = ra->base;
  memset(&a, 0, sizeof(a));
  a.out = d_out;
  a.spheres = d_spheres;
  a.rng_state = nullptr;  // the session's own generator: seeded at sample 0, the record's afterwards
  memcpy(a.basis, basis, sizeof(a.basis));
  memcpy(a.eye, eye, sizeof(a.eye));
  a.n_spheres = n_spheres;
  a.width = r->width;
  a.height = r->height;
  a.row_begin = r->opts.row_begin;
  a.tile_pixels = r->tile_pixels;
  a.spp = (int32_t)(p->samples + spp);  // the frame this pass completes
  a.max_bounces = r->opts.max_bounces;
  a.frame = 0u;
  a.planar = r->opts.layout == PT_LAYOUT_PLANAR ? 1u : 0u;
  a.fail_count = nullptr;
  a.accel = r->d_accel;
  a.seed = r->opts.seed;
  a.err_word = r->d_err;
  a.chunk_wait_ticks = r->chunk_wait_ticks;
  a.debug = r->debug;
  a.vertices = nullptr;  // (display vertices: pt_display_pack on the frame)
  a.prio = (spp >= 4 && (uint64_t)r->tile_pixels <= 2u * r->resident_pixels) ? 1u : 0u;  // as fill_args, on the pass's own count
  ra->sample_begin = (int32_t)p->samples;
  ra->session = p->d_rec;
  return PT_OK;
}

// the pass went out: the session now holds its samples (and, after its first pass, its camera and scene)
static void progressive_advance(pt_progressive* p, int spp, const pt_sphere* d_spheres, int n_spheres, const float basis[12], const float eye[3]) {
  if (p->samples == 0) {
    memcpy(p->cam, basis, 12 * sizeof(float));
    memcpy(p->cam + 12, eye, 3 * sizeof(float));
    p->spheres = d_spheres;
    p->n_spheres = n_spheres;
  }
  p->samples += spp;
}

// The pass's launches: a plain session's one resume launch; an adaptive session's selection, the pass over its list and the frame
static int launch_progressive_pass(pt_progressive* p, const ResumeKernelArgs& ra, int variant, hipStream_t stream) {
  pt_renderer* r = p->r;
  if (!p->d_adaptive) {
    PT_HIP(pt_launch_resume_kernel(ra, r->opts.rng_mode, variant, stream));
    return PT_OK;
  }
  const int mode = p->forced ? 1 : (p->samples == 0 ? 2 : 0);
  PT_HIP(pt_launch_adaptive_select(p->ast, p->rule, p->d_rec, r->tile_pixels, r->width, (int)p->samples, ra.base.spp, mode, false, stream));
  AdaptiveKernelArgs aa;
  static_cast<ResumeKernelArgs&>(aa) = ra;
  aa.list = p->ast.list;
  aa.list_len = p->ast.words;
  PT_HIP(pt_launch_adaptive_kernel(aa, r->opts.rng_mode, variant, stream));
  PT_HIP(pt_launch_adaptive_finalize(p->d_rec, p->ast.counts, ra.base.out, r->tile_pixels, r->opts.layout == PT_LAYOUT_PLANAR, stream));
  p->forced = false;
  return PT_OK;
}

int pt_progressive_enqueue(pt_progressive* p, int spp, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                           const float eye[3], void* hip_stream) {
  ResumeKernelArgs ra;
  int variant = 0;
  int rc = progressive_args(p, spp, d_out, d_spheres, n_spheres, basis, eye, &ra, &variant);
  if (rc != PT_OK) return rc;
  pt_renderer* r = p->r;
  if (r->tile_pixels) {
    const hipStream_t stream = (hipStream_t)hip_stream;
    rc = order_after_last(r, stream);  // (the grid buffer is the renderer's)
    if (rc != PT_OK) return rc;
    rc = launch_progressive_pass(p, ra, variant, stream);
    if (rc != PT_OK) return rc;
    rc = mark_last(r, stream);
    if (rc != PT_OK) return rc;
  }
  progressive_advance(p, spp, d_spheres, n_spheres, basis, eye);
  return PT_OK;
}

int pt_progressive_render(pt_progressive* p, int spp, float* d_out, const pt_sphere* d_spheres, int n_spheres, const float basis[12],
                          const float eye[3], float* ms_out) {
  ResumeKernelArgs ra;
  int variant = 0;
  if (ms_out) *ms_out = 0.0f;
  int rc = progressive_args(p, spp, d_out, d_spheres, n_spheres, basis, eye, &ra, &variant);
  if (rc != PT_OK) return rc;
  pt_renderer* r = p->r;
  if (r->tile_pixels) {
    rc = order_after_last(r, nullptr);
    if (rc != PT_OK) return rc;
    PT_HIP(hipEventRecord(p->ev_start, nullptr));
    rc = launch_progressive_pass(p, ra, variant, nullptr);
    if (rc != PT_OK) return rc;
    PT_HIP(hipEventRecord(p->ev_stop, nullptr));
    PT_HIP(hipEventSynchronize(p->ev_stop));
    r->have_last = false;  // the pass has completed: nothing left to order against
    float ms = 0.0f;
    PT_HIP(hipEventElapsedTime(&ms, p->ev_start, p->ev_stop));
    if (ms_out) *ms_out = ms;
  }
  progressive_advance(p, spp, d_spheres, n_spheres, basis, eye);
  return PT_OK;
}

int pt_progressive_set_adaptive(pt_progressive* p, const pt_adaptive_opts* opts) {
  if (!p) return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: session is NULL");
  if (p->samples != 0) return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: the session holds %lld samples: only at 0 samples (reset it)", (long long)p->samples);
  if (opts) {
    if (!(opts->tolerance >= 0.0f)) return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: tolerance %g (>= 0)", (double)opts->tolerance);
    if (!(opts->floor > 0.0f)) return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: floor %g (> 0)", (double)opts->floor);
    if (opts->min_samples < 2) return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: min_samples %d (>= 2)", opts->min_samples);
    if (opts->radius < 0 || opts->radius > PT_ADAPTIVE_MAX_RADIUS)
      return pt_fail(PT_EINVAL, "pt_progressive_set_adaptive: radius %d (0..%d)", opts->radius, PT_ADAPTIVE_MAX_RADIUS);
  }
  if (!opts) {  // off: a plain session again
    if (p->d_adaptive) (void)hipFree(p->d_adaptive);
    p->d_adaptive = nullptr;
    memset(&p->ast, 0, sizeof(p->ast));
    p->forced = false;
    return PT_OK;
  }
  const uint32_t tp = p->r->tile_pixels;
  if (!p->d_adaptive && tp) {
    const size_t n_blocks = (tp + PT_ADAPTIVE_BLOCK - 1) / PT_ADAPTIVE_BLOCK;
    const size_t words = 2 * (size_t)tp + n_blocks + 4;  // counts, list, block sums, words; then the mask bytes
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, words * sizeof(uint32_t) + tp);
    if (e != hipSuccess) return pt_fail(e == hipErrorNoDevice ? PT_ENODEVICE : PT_EHIP, "pt_progressive_set_adaptive: %s", hipGetErrorString(e));
    uint32_t* w = (uint32_t*)d;
    p->d_adaptive = d;
    p->ast.counts = w;
    p->ast.list = w + tp;
    p->ast.block_sums = w + 2 * (size_t)tp;
    p->ast.words = w + 2 * (size_t)tp + n_blocks;
    p->ast.mask = (uint8_t*)(w + words);
    PT_HIP(hipMemset(p->ast.words, 0, 4 * sizeof(uint32_t)));
  }
  p->opts = *opts;
  p->rule = pt_adaptive_rule(*opts);
  p->forced = false;
  return PT_OK;
}

int pt_progressive_active(pt_progressive* p, int64_t* active) {
  if (!p || !active) return pt_fail(PT_EINVAL, "pt_progressive_active: NULL argument");
  pt_renderer* r = p->r;
  *active = (int64_t)r->tile_pixels;
  if (!p->d_adaptive || p->samples == 0 || !r->tile_pixels) return PT_OK;  // (a first pass renders every pixel)
  int rc = order_after_last(r, nullptr);
  if (rc != PT_OK) return rc;
  // the next pass's decision without its list: the selection's first three steps (they only rewrite the scratch bits)
  PT_HIP(pt_launch_adaptive_select(p->ast, p->rule, p->d_rec, r->tile_pixels, r->width, (int)p->samples, (int)p->samples + 1,
                                   p->forced ? 1 : 0, true, nullptr));
  uint32_t n = 0u;
  PT_HIP(hipMemcpy(&n, p->ast.words, sizeof(n), hipMemcpyDeviceToHost));
  r->have_last = false;  // (the copy waited for everything before it on the default stream)
  *active = (int64_t)n;
  return PT_OK;
}

int pt_progressive_counts(pt_progressive* p, uint32_t* d_counts, void* hip_stream) {
  if (!p) return pt_fail(PT_EINVAL, "pt_progressive_counts: session is NULL");
  pt_renderer* r = p->r;
  if (!r->tile_pixels) return PT_OK;
  if (!d_counts) return pt_fail(PT_EINVAL, "pt_progressive_counts: d_counts is NULL");
  if (p->samples > (int64_t)UINT32_MAX) return pt_fail(PT_EINVAL, "pt_progressive_counts: count beyond 32 bits");
  const hipStream_t stream = (hipStream_t)hip_stream;
  int rc = order_after_last(r, stream);
  if (rc != PT_OK) return rc;
  if (p->d_adaptive && p->samples > 0)
    PT_HIP(hipMemcpyAsync(d_counts, p->ast.counts, (size_t)r->tile_pixels * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
  else
    PT_HIP(hipMemsetD32Async((hipDeviceptr_t)d_counts, (int)p->samples, r->tile_pixels, stream));
  return mark_last(r, stream);  // (a later pass rewrites the counts: it waits for the copy)
}

#if PT_BUILD_EXPERIMENTS
// lab library: a copy of the session's record, PT_CHUNK_WORDS words per tile pixel, [word][pixel] (include/ptcore_lab.h)
int pt_debug_progressive_record(pt_progressive* p, uint32_t* host) {
  if (!p || !host) return pt_fail(PT_EINVAL, "pt_debug_progressive_record: NULL argument");
  if (!p->r->tile_pixels) return PT_OK;
  int rc = session_sync(p);
  if (rc != PT_OK) return rc;
  PT_HIP(hipMemcpy(host, p->d_rec, (size_t)PT_CHUNK_WORDS * p->r->tile_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PT_OK;
}

// lab library: the next pass renders exactly the pixels of host_mask (one byte per tile pixel, non-zero = active); the set may only
// shrink (a pixel the last pass did not render cannot come back)
int pt_debug_progressive_set_active(pt_progressive* p, const uint8_t* host_mask) {
  if (!p || !host_mask) return pt_fail(PT_EINVAL, "pt_debug_progressive_set_active: NULL argument");
  if (!p->d_adaptive) return pt_fail(PT_EINVAL, "pt_debug_progressive_set_active: not an adaptive session");
  if (p->samples == 0) return pt_fail(PT_EINVAL, "pt_debug_progressive_set_active: a first pass renders every pixel");
  const uint32_t tp = p->r->tile_pixels;
  if (!tp) return PT_OK;
  int rc = session_sync(p);
  if (rc != PT_OK) return rc;
  uint8_t* m = (uint8_t*)malloc(tp);
  if (!m) return pt_fail(PT_ENOMEM, "pt_debug_progressive_set_active: out of host memory");
  hipError_t e = hipMemcpy(m, p->ast.mask, tp, hipMemcpyDeviceToHost);
  bool grows = false;
  for (uint32_t i = 0; e == hipSuccess && i < tp; i++) {
    const uint8_t want = host_mask[i] ? 1u : 0u;
    if (want && !(m[i] & 1u)) grows = true;
    m[i] = want;
  }
  if (e == hipSuccess && !grows) e = hipMemcpy(p->ast.mask, m, tp, hipMemcpyHostToDevice);
  free(m);
  if (e != hipSuccess) return pt_fail(PT_EHIP, "pt_debug_progressive_set_active: %s", hipGetErrorString(e));
  if (grows) return pt_fail(PT_EINVAL, "pt_debug_progressive_set_active: the set may only shrink");
  p->forced = true;
  return PT_OK;
}
#endif

#if PT_BUILD_EXPERIMENTS
// lab library: a session's sample count without the samples (the INT_MAX limit's test, include/ptcore_lab.h)
int pt_debug_progressive_set_samples(pt_progressive* p, int64_t samples) {
  if (!p || samples < 0) return pt_fail(PT_EINVAL, "pt_debug_progressive_set_samples: bad arguments");
  p->samples = samples;
  return PT_OK;
}
#endif

#if PT_BUILD_EXPERIMENTS
// lab library: the variant the C++ policy itself picks for a tile of the reference's scene (tests/test_policy_model.py compares
// it with the Python restatement of the argmin)
int pt_debug_policy_choice(int rng_mode, double waves_per_simd, int spp, int bounces, int with9, int chunked, int* variant) {
  if (!variant) return pt_fail(PT_EINVAL, "pt_debug_policy_choice: variant is NULL");
  *variant = cheapest_variant(rng_mode, waves_per_simd, spp, bounces, with9 != 0, chunked ? ((1u << 6) | (1u << 8) | (1u << 9)) : 0u);
  return PT_OK;
}
// lab library: the policy's cost model, for tests/test_policy_model.py (include/ptcore_lab.h)
int pt_debug_policy_ms(int rng_mode, int variant, double waves_per_simd, int spp, int bounces, double* ms) {
  if (!ms) return pt_fail(PT_EINVAL, "pt_debug_policy_ms: ms is NULL");
  for (const KernelCost& c : kKernelCost[rng_mode == PT_RNG_PHILOX ? 1 : 0])
    if (c.variant == variant) {
      *ms = predicted_ms(c, waves_per_simd, spp, bounces, spp >= 512);
      return PT_OK;
    }
  return pt_fail(PT_EINVAL, "pt_debug_policy_ms: no cost record for variant %d", variant);
}
#endif

int pt_renderer_set_display(pt_renderer* r, float* d_vertices) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_set_display: renderer is NULL");
  r->d_vertices = d_vertices;
  return PT_OK;
}

// ---- sphere materials (include/ptcore.h; the kernel: pt_materials.hip) -------------------------------------------------------
int pt_material_check(const pt_material* table, int n) {
  if (!table) return pt_fail(PT_EINVAL, "pt_material_check: table is NULL");
  if (n < 1) return pt_fail(PT_EINVAL, "pt_material_check: n %d (a table has one entry per sphere; NULL, 0 clears a renderer's)", n);
  if (n > PT_MATERIALS_MAX_SPHERES)
    return pt_fail(PT_ELIMIT, "pt_material_check: n %d exceeds the %d spheres the materials kernel stages", n, PT_MATERIALS_MAX_SPHERES);
  for (int i = 0; i < n; i++) {
    const int kind = table[i].kind;
    const float p = table[i].param;
    if (kind < PT_MATERIAL_DIFFUSE || kind > PT_MATERIAL_GLASS) return pt_fail(PT_EINVAL, "pt_material_check: table[%d].kind %d (0 .. 3)", i, kind);
    if (!isfinite(p)) return pt_fail(PT_EINVAL, "pt_material_check: table[%d].param is not finite", i);
    if ((kind == PT_MATERIAL_DIFFUSE || kind == PT_MATERIAL_MIRROR) && p != 0.0f)
      return pt_fail(PT_EINVAL, "pt_material_check: table[%d].param %g (%s takes 0)", i, (double)p, kind == PT_MATERIAL_DIFFUSE ? "DIFFUSE" : "MIRROR");
    if (kind == PT_MATERIAL_GLOSSY && !(p > 0.0f && p < 1.0f))
      return pt_fail(PT_EINVAL, "pt_material_check: table[%d].param %g (GLOSSY roughness: 0 < rho < 1)", i, (double)p);
    if (kind == PT_MATERIAL_GLASS && !(p > 1.0f && p <= 4.0f))
      return pt_fail(PT_EINVAL, "pt_material_check: table[%d].param %g (GLASS index of refraction: 1 < eta <= 4)", i, (double)p);
  }
  return PT_OK;
}

int pt_renderer_set_materials(pt_renderer* r, const pt_material* host_table, int n) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_set_materials: renderer is NULL");
  const bool clear = !host_table && n == 0;
  if (!clear) {
    if (r->opts.fast_math) return pt_fail(PT_EINVAL, "pt_renderer_set_materials: a fast_math renderer has no materials");
    if (!r->auto_variant)
      return pt_fail(PT_EINVAL, "pt_renderer_set_materials: the renderer has an explicit kernel variant (%d); the materials kernel is none of the table's: leave variant at -1", r->opts.variant);
    const int rc = pt_material_check(host_table, n);
    if (rc != PT_OK) return rc;
  }
  PT_HIP(hipDeviceSynchronize());  // no frame in flight reads the table that goes
  if (r->d_materials) {
    void* old = r->d_materials;
    r->d_materials = nullptr;
    r->n_materials = 0;
    PT_HIP(hipFree(old));
  }
  if (clear) return PT_OK;
  unsigned char* rows = new (std::nothrow) unsigned char[(size_t)n * 16];
  if (!rows) return pt_fail(PT_ENOMEM, "pt_renderer_set_materials: out of host memory");
  for (int i = 0; i < n; i++) pt_materials_device_row(host_table + i, rows + (size_t)i * 16);
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, (size_t)n * 16);
  if (e == hipSuccess) e = hipMemcpy(d, rows, (size_t)n * 16, hipMemcpyHostToDevice);
  delete[] rows;
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return pt_fail(PT_EHIP, "pt_renderer_set_materials: %s", hipGetErrorString(e));
  }
  r->d_materials = d;
  r->n_materials = n;
  return PT_OK;
}

// the table of a renderer without one: every sphere DIFFUSE (kind 0, param 0: zeroed rows)
static int ensure_all_diffuse(pt_renderer* r, const char* who) {
  if (r->d_all_diffuse) return PT_OK;
  static const unsigned char zeros[PT_MATERIALS_MAX_SPHERES * 16] = {};
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, sizeof(zeros));
  if (e == hipSuccess) e = hipMemcpy(d, zeros, sizeof(zeros), hipMemcpyHostToDevice);  // blocking, like set_materials' upload
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return pt_fail(PT_EHIP, "%s: %s", who, hipGetErrorString(e));
  }
  r->d_all_diffuse = d;
  return PT_OK;
}

int pt_renderer_set_light_sampling(pt_renderer* r, int on) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_set_light_sampling: renderer is NULL");
  if (!on) {
    r->light_sampling = false;  // the table, if any, stays: PT_VARIANT_MATERIALS with one, the ordinary kernels without
    return PT_OK;
  }
  if (r->opts.fast_math) return pt_fail(PT_EINVAL, "pt_renderer_set_light_sampling: a fast_math renderer has no light sampling");
  if (!r->auto_variant)
    return pt_fail(PT_EINVAL, "pt_renderer_set_light_sampling: the renderer has an explicit kernel variant (%d); the light-sampling kernel is none of the table's: leave variant at -1", r->opts.variant);
  const int rc = ensure_all_diffuse(r, "pt_renderer_set_light_sampling");
  if (rc != PT_OK) return rc;
  r->light_sampling = true;
  return PT_OK;
}

// ---- sky and sun (include/ptcore.h; EXACTNESS.md A.24) -------------------------------------------------------------------------
int pt_sky_check(const pt_sky* sky) {
  if (!sky) return pt_fail(PT_EINVAL, "pt_sky_check: sky is NULL");
  const struct { const char* name; const float* v; } rad[4] = {{"zenith", sky->zenith}, {"horizon", sky->horizon}, {"ground", sky->ground},
                                                                {"sun_radiance", sky->sun_radiance}};
  for (const auto& f : rad)
    for (int k = 0; k < 3; k++) {
      if (!isfinite(f.v[k])) return pt_fail(PT_EINVAL, "pt_sky_check: %s[%d] is not finite", f.name, k);
      if (f.v[k] < 0.0f) return pt_fail(PT_EINVAL, "pt_sky_check: %s[%d] %g is negative (a radiance)", f.name, k, (double)f.v[k]);
    }
  const bool sun = sky->sun_radiance[0] > 0.0f || sky->sun_radiance[1] > 0.0f || sky->sun_radiance[2] > 0.0f;
  if (!sun) return PT_OK;
  for (int k = 0; k < 3; k++)
    if (!isfinite(sky->sun_dir[k])) return pt_fail(PT_EINVAL, "pt_sky_check: sun_dir[%d] is not finite", k);
  // the length the host normalises by, in float32 as pt_materials_sky_consts forms it: it must be a finite, non-zero number
  const float len2 = sky->sun_dir[0] * sky->sun_dir[0] + sky->sun_dir[1] * sky->sun_dir[1] + sky->sun_dir[2] * sky->sun_dir[2];
  if (!(len2 > 0.0f) || !isfinite(len2) || !isfinite(1.0f / sqrtf(len2)))
    return pt_fail(PT_EINVAL, "pt_sky_check: sun_dir (%g, %g, %g) has no direction (zero length, or a squared length float32 cannot hold)",
                   (double)sky->sun_dir[0], (double)sky->sun_dir[1], (double)sky->sun_dir[2]);
  if (!(sky->sun_cos >= 0.0f && sky->sun_cos < 1.0f))
    return pt_fail(PT_EINVAL, "pt_sky_check: sun_cos %g (the cosine of the sun's angular radius: 0 <= sun_cos < 1)", (double)sky->sun_cos);
  if (1.0f - sky->sun_cos < 9.5367431640625e-07f)
    return pt_fail(PT_EINVAL, "pt_sky_check: sun_cos %.9g is too near 1 (1 - sun_cos must be at least 2^-20)", (double)sky->sun_cos);
  return PT_OK;
}

int pt_renderer_set_sky(pt_renderer* r, const pt_sky* sky) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_set_sky: renderer is NULL");
  if (!sky) {
    r->has_sky = false;  // the table and light sampling, if any, stay: the renderer is what it was before the sky
    return PT_OK;
  }
  if (r->opts.fast_math) return pt_fail(PT_EINVAL, "pt_renderer_set_sky: a fast_math renderer has no sky");
  if (!r->auto_variant)
    return pt_fail(PT_EINVAL, "pt_renderer_set_sky: the renderer has an explicit kernel variant (%d); the sky kernel is none of the table's: leave variant at -1", r->opts.variant);
  int rc = pt_sky_check(sky);
  if (rc != PT_OK) return rc;
  rc = ensure_all_diffuse(r, "pt_renderer_set_sky");
  if (rc != PT_OK) return rc;
  pt_materials_sky_consts(sky, &r->sky);  // by value into every launch: a frame in flight keeps the constants it was launched with
  r->has_sky = true;
  return PT_OK;
}

int pt_renderer_set_frame(pt_renderer* r, uint32_t frame) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_set_frame: renderer is NULL");
  r->frame = frame;
  return PT_OK;
}

int pt_renderer_reset_rng(pt_renderer* r) {
  if (!r) return pt_fail(PT_EINVAL, "pt_renderer_reset_rng: renderer is NULL");
  r->frame = 0;
  return setup_random(r);
}

int pt_renderer_get_rng_state(pt_renderer* r, uint32_t* h_state, size_t n_words) {
  if (!r || !h_state) return pt_fail(PT_EINVAL, "pt_renderer_get_rng_state: NULL argument");
  if (!r->d_state) return pt_fail(PT_EINVAL, "pt_renderer_get_rng_state: renderer keeps no generator state");
  if (n_words != (size_t)r->tile_pixels * 6) return pt_fail(PT_EINVAL, "pt_renderer_get_rng_state: expected %zu words", (size_t)r->tile_pixels * 6);
  PT_HIP(hipMemcpy(h_state, r->d_state, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_renderer_set_rng_state(pt_renderer* r, const uint32_t* h_state, size_t n_words) {
  if (!r || !h_state) return pt_fail(PT_EINVAL, "pt_renderer_set_rng_state: NULL argument");
  if (!r->d_state) return pt_fail(PT_EINVAL, "pt_renderer_set_rng_state: renderer keeps no generator state");
  if (n_words != (size_t)r->tile_pixels * 6) return pt_fail(PT_EINVAL, "pt_renderer_set_rng_state: expected %zu words", (size_t)r->tile_pixels * 6);
  PT_HIP(hipMemcpy(r->d_state, h_state, n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
  return PT_OK;
}

int pt_renderer_kernel_info(pt_renderer* r, int n_spheres, pt_kernel_info* info) {
  if (!r || !info) return pt_fail(PT_EINVAL, "pt_renderer_kernel_info: NULL argument");
  hipFuncAttributes fa;
  const int variant = effective_variant(r, n_spheres);
  if (materials_variant(variant)) {
    PT_HIP(hipFuncGetAttributes(&fa, pt_materials_kernel_symbol(r->opts.rng_mode, lights_variant(variant), sky_variant(variant))));
    info->block_threads = PT_BLOCK_THREADS;
    info->grid_blocks = (int)(((uint64_t)r->tile_pixels + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS);
    info->lds_bytes = (int)pt_materials_kernel_lds_bytes(n_spheres < 0 ? 0 : (n_spheres > PT_MATERIALS_MAX_SPHERES ? PT_MATERIALS_MAX_SPHERES : n_spheres));
    info->variant = variant;
    info->num_vgprs = fa.numRegs;
    info->reserved0 = 0;
    info->scratch_bytes = (int)fa.localSizeBytes;
    info->max_spheres = PT_MATERIALS_MAX_SPHERES;
    return PT_OK;
  }
  const bool fast = variant == PT_VARIANT_FAST;
  PT_HIP(hipFuncGetAttributes(&fa, fast ? pt_fast_kernel_symbol(r->opts.rng_mode, n_spheres, r->opts.max_bounces)
                                        : pt_kernel_symbol(r->opts.rng_mode, variant, n_spheres, r->opts.max_bounces,
                                                           r->opts.layout == PT_LAYOUT_PLANAR)));
  const int block = fast ? PT_BLOCK_THREADS : pt_kernel_block_threads(variant);
  const int lanes = fast ? 1 : pt_kernel_variant(variant).lanes;  // per pixel
  info->block_threads = block;
  info->grid_blocks = (int)(((uint64_t)r->tile_pixels * (uint64_t)lanes + block - 1) / block);
  info->lds_bytes = (int)(fast ? pt_fast_kernel_lds_bytes(n_spheres) : pt_kernel_lds_bytes(n_spheres, variant));
  info->variant = variant;
  if (!fast && chunks_of(r, variant) >= 2u &&
      pt_kernel_chunked(variant, n_spheres, r->opts.max_bounces, r->opts.layout == PT_LAYOUT_PLANAR, r->spp, chunks_of(r, variant)))
    info->grid_blocks *= (int)chunks_of(r, variant);  // sample chunking: that many workgroups per pixel block
  info->num_vgprs = fa.numRegs;
  info->reserved0 = 0;
  info->scratch_bytes = (int)fa.localSizeBytes;
  info->max_spheres = fast ? (1 << 26) : pt_kernel_max_spheres(variant);
  return PT_OK;
}

}  // extern "C"
