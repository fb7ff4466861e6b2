/*
 * ptcore_lab.h -- additional exports of libptcore_lab.so, the LAB build of the same sources
 * (csrc/Makefile, -DPT_BUILD_EXPERIMENTS=1): everything in ptcore.h, plus the experimental kernel
 * variants 1-5, 7, 11 and 12 (stepping stones, superseded kernels and measured negative results, HISTORY.md B.2) and the
 * diagnostic entry points below.  Loaded by the variant / exhaustive tests and the tools; the
 * product library libptcore.so exports none of this.  No reference counterpart.
 */
#ifndef PTCORE_LAB_H
#define PTCORE_LAB_H

#include "ptcore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scalar building blocks of the device code, evaluated elementwise on the GPU. */
enum {
  PT_FN_INV_SQRT_LITERAL = 0, /* 1.0f / sqrtf(x): helper_math normalize's rsqrtf (contract C2) */
  PT_FN_INV_SQRT_FAST = 1,    /* the 7-instruction sequence the kernel uses for the same value   */
  PT_FN_SQRT_LITERAL = 2,     /* sqrtf(x)                                                        */
  PT_FN_SQRT_FAST = 3,        /* 5-instruction correctly rounded sqrt                             */
  PT_FN_SIN = 4,              /* contract C4 sin on (0, 2*pi], the kernels' instruction sequence  */
  PT_FN_COS = 5,              /* contract C4 cos                                                  */
  PT_FN_UNIFORM = 6,          /* curand_uniform mapping of the argument's BIT PATTERN             */
  PT_FN_ONEMINUS_LITERAL = 7, /* (float)sqrt(1.0 - (double)(x*x)), pathtrace.cu:134               */
  PT_FN_ONEMINUS_FAST = 8,    /* same through the lean correctly rounded double sqrt              */
  PT_FN_ONEMINUS_F32 = 9,     /* the same without FP64 (pt_device.h, oneminus_f32_nb), the literal where it flags itself */
  PT_FN_ONEMINUS_F32_FLAG = 10, /* 1.0f where oneminus_f32_nb flags itself, else 0.0f                              */
  PT_FN_ZERO = 11,
  PT_FN_UNIFORM_LITERAL = 12, /* curand_uniform as multiply, then add (the kernels use the equivalent single fma) */
  PT_FN_SIN_LITERAL = 13,     /* contract C4 as the oracle writes it (rintf, int conversion, selects); PT_FN_SIN/COS are the  */
  PT_FN_COS_LITERAL = 14,     /* kernels' form of the same floats (magic-number rounding, bit selections)                     */
  PT_FN_COUNT = 15
};
int pt_debug_unary_map(int fn, const float* d_in, float* d_out, size_t n);
/* Compare fn_a and fn_b on the `count` consecutive float bit patterns starting at first_bits
 * (count <= 2^32); NaN results compare equal.  *n_mismatch = number of differing inputs. */
int pt_debug_unary_compare(int fn_a, int fn_b, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch,
                           uint32_t* example_bits);
/* The Welford update's division by the sample count (pathtrace.cu:52) as the kernels evaluate it -- reciprocal from a table,
 * exact remainder, one correction (pt_device.h, div_by_count) -- against the division itself, for the counts
 * n_first .. n_first + n_count - 1 and the `count` consecutive float bit patterns of the dividend starting at first_bits.
 * *n_mismatch = number of (count, dividend) pairs whose quotients differ in any bit (NaN == NaN). */
int pt_debug_div_compare(uint32_t n_first, uint32_t n_count, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch,
                         uint32_t* example_bits, uint32_t* example_n);
/* Diagnostics: builds the uniform grid of kernel variant 11 for a scene and returns its 64-byte header
 * {valid, nx, ny, nz, origin xyz, cell size, 1/cell size, slack, centre xyz, (2E)^2, n_big, n_items}. */
int pt_debug_grid_header(const pt_sphere* d_spheres, int n_spheres, uint32_t header_out[16]);
/* Diagnostics: the whole image the grid builder writes for a scene, as the many-sphere kernel with `threads`-wide workgroups (512
 * or 1024) would get it; `eye` = camera hint or NULL.  layout_out = {image bytes, byte offsets of: out-of-grid list (u16), cell
 * starts (u16, cells + 2), registrations (u16), pooled cell table (2 x u32 per entry), emission data; cells the starts have room
 * for; entries the pooled table may have}.  image_out NULL: only the layout is returned. */
int pt_debug_grid_image(const pt_sphere* d_spheres, int n_spheres, const float* eye, int threads, uint32_t* image_out,
                        size_t image_bytes, uint64_t layout_out[8]);
/* The pixel-footprint analysis alone (csrc/pt_footprint.h, primary_candidates): one lane per pixel of rows [row_begin, row_end) in
 * the pixel kernels' order (tile pixel tp: row = row_begin + tp / width, col = tp % width), the scene (1 .. 64 spheres) staged as
 * the reference-configuration builds stage it.  d_masks[tp] = the lane's OWN word (bit j = sphere j is kept), not the wave's
 * union; d_dirs (may be NULL) = the five directions the lane used, [pixels][5][3] floats: the centre, then the corners
 * (row -+ 0.5, col -+ 0.5) with the row's sign changing fastest.  eye[3] and basis[12] are host arrays, d_* device.  Synchronous. */
int pt_debug_primary_masks(const pt_sphere* d_spheres, int n_spheres, const float eye[3], const float basis[12], int width, int height,
                           int row_begin, int row_end, uint32_t* d_masks, float* d_dirs);
/* The per-pixel primary-ray lists alone (csrc/pt_primlist.h, build_primary_list).  Builds the grid exactly as
 * pt_debug_grid_image does (eye as the camera hint, `threads` = 512 or 1024) and returns its 20 header words in header_out
 * (host; word 0 = valid).  On a valid grid, workgroups of `threads` lanes with the pooled kernel's LDS layout each build their
 * lanes' lists, lane L of the launch = tile pixel L; d_lists gets six words per LANE -- the tile rounded up to a multiple of
 * `threads`, the lanes past the tile being the inactive ones --: {list valid, length, then the two table entries e0.x, e0.y,
 * e1.x, e1.y read back from the lane's slots prim_base + 2 * lane-in-workgroup (csrc/pt_grid.h has the entry format)}.  An
 * invalid grid (header_out[0] == 0) is no error: nothing is launched and d_lists is left alone.  Synchronous. */
int pt_debug_primary_lists(const pt_sphere* d_spheres, int n_spheres, const float eye[3], const float basis[12], int width, int height,
                           int row_begin, int row_end, int threads, uint32_t* d_lists, uint32_t header_out[20]);
/* The automatic policy's cost model (csrc/pt_capi.hip, "which kernel for a small scene"): predicted kernel milliseconds of
 * variant 6, 8 or 9 on a tile of `waves_per_simd` one-lane waves per SIMD at `spp` samples and `bounces` bounces.  Host
 * arithmetic only (no device needed): tests/test_policy_model.py holds it against the measured sweeps under profiles/. */
int pt_debug_policy_ms(int rng_mode, int variant, double waves_per_simd, int spp, int bounces, double* ms);
/* the variant the library's own cost-model policy picks (6, 8 or 9) for a tile of `waves_per_simd` one-lane waves per SIMD */
int pt_debug_policy_choice(int rng_mode, double waves_per_simd, int spp, int bounces, int with9, int chunked, int* variant);
/* *launches = the launches of the frames kernel (one per group of up to 32 frames) that pt_renderer_enqueue_frames has made on
 * this renderer since it was created; frames that went out as single enqueues do not count.  The tests of the batch kernel
 * use it to see that the kernel they check is the one that ran. */
int pt_debug_renderer_batch_launches(pt_renderer* r, uint32_t* launches);

/* The builds behind the kernel selectors: every distinct kernel function that the pixel-kernel selector (csrc/pt_kernel.hip,
 * select_kernel) and the fast mode's (csrc/pt_fast.hip) can return in this library, found by walking the selectors themselves.
 * *n_builds = their number (info may be NULL); info = {flavour (0 plain, 1 frames, 2 resume, 3 adaptive, 4 fast), generator
 * (PT_RNG_*), kernel row (100 for the fast mode; a wide row reports the row whose kernel it runs), wide, lean LDS layout,
 * reference bounces (0 generic, 5, 8), lanes per pixel, the first table row that selects it}.  Host only: needs no device. */
#define PT_BUILD_INFO_WORDS 8
int pt_debug_kernel_builds(int index, int* n_builds, int32_t info[PT_BUILD_INFO_WORDS]);
/* Row `row` of the kernel-variant table (csrc/pt_kernel.h, VariantInfo): info = {product, lanes, threads, lean (0 never, 1 above
 * 10 spheres, 2 always), grid, wide, ref_builds, resume, frames, can_chunk, kernel, chunk_family}; *n_rows = rows.  Host only. */
#define PT_ROW_INFO_WORDS 12
int pt_debug_variant_row(int row, int* n_rows, int32_t info[PT_ROW_INFO_WORDS]);
/* The launch census.  Every launcher of a pixel kernel counts each launch that succeeded under the function it launched:
 * *launches = launches of build `index` (the index of pt_debug_kernel_builds) since the last reset, by any renderer and thread
 * of the process; *modes = the OR over those launches of what each was (PT_CENSUS_* below).  index -1: launches of functions
 * that are not in the list (there should be none).  The tests use it to see that the build they compare is the one that ran. */
enum {
  PT_CENSUS_MODE_CHUNKED = 1,     /* the samples were chained through chunks > 1 workgroups                                */
  PT_CENSUS_MODE_REPAIR = 2,      /* a repair launch after a broken chunk chain                                            */
  PT_CENSUS_MODE_PLANAR = 4,      /* channel-first output                                                                  */
  PT_CENSUS_MODE_VERTICES = 8,    /* the fused display vertices were written                                               */
  PT_CENSUS_MODE_RNG_STATE = 16,  /* a persisted generator state was read and written (else: seeded in the kernel)         */
  PT_CENSUS_MODE_FOOTPRINT = 32,  /* the build has the pixel-footprint analysis and the launch's sample count reached it   */
  PT_CENSUS_MODE_FIRST_PASS = 64, /* resume and adaptive builds: the pass started from zero samples                        */
  PT_CENSUS_MODE_PRIO = 128       /* issue priority by progress was on                                                     */
};
int pt_debug_launch_census(int index, uint32_t* launches, uint32_t* modes);
int pt_debug_launch_census_reset(void);

/* The fast mode's scene intersection on a list of rays (csrc/pt_fast.hip, nearest<>): what no frame shows per ray -- the LAST
 * shortcut (the key alone decides; only the last bounce of the 9-sphere, 5-bounce build uses it) and the masked loop of the
 * specialised build (only primary rays at spp >= 8 reach it).  d_rays holds n_rays rays of 6 floats {o, d}.  specialised != 0
 * requires n_spheres == 9 and runs nearest<9, .>, else nearest<0, .>; last = 0 or 1; mask = the spheres to rank (bit i = sphere
 * i; the generic build ranks all of them whatever it says).  The scene is staged as the frame kernel stages it (LDS up to 64
 * spheres, read in place above), one ray per thread of 256-thread workgroups.  Per ray: d_t = the t nearest<> reports (with
 * last: the ranked key, index bits cleared), d_idx = the sphere, -1 for a miss.  Synchronous. */
int pt_debug_fast_nearest(const pt_sphere* d_spheres, int n_spheres, const float* d_rays, uint32_t n_rays, int specialised, int last,
                          uint32_t mask, float* d_t, int32_t* d_idx);

/* Denoiser diagnostics (csrc/pt_denoise.hip).  Layers = the activation buffers of the workspace, in execution order:
 * 0 "input" (the pre-processed frame, NHWC, 16 channels of which 14-15 are zero), "block<b>.t1" / ".res" / ".out", "lat6",
 * "back<k+1><k>", "rep<k>".  shape = {rows, cols, channels}; *n_layers = their number (also for an invalid `layer`). */
int pt_debug_denoiser_layer_info(pt_denoiser* d, int layer, int* n_layers, int shape[3], char* name, size_t name_len);
/* Synchronises the device and copies layer `layer` ([rows][cols][channels] floats, n_floats of them) to / from the host.  With
 * reserved batches the workspace holds [max_frames] copies of every layer; these address the first (the frame of a
 * single enqueue, or the first frame of the last group). */
int pt_debug_denoiser_activation(pt_denoiser* d, int layer, float* h_out, size_t n_floats);
int pt_debug_denoiser_set_activation(pt_denoiser* d, int layer, const float* h_in, size_t n_floats);
/* The same for the first `frames` frames of the layer, [frames][rows][cols][channels] from the layer's offset (contiguous
 * whatever max_frames the workspace was laid out for).  frames outside 1 .. max_frames: PT_EINVAL. */
int pt_debug_denoiser_activation_frames(pt_denoiser* d, int layer, int frames, float* h_out, size_t n_floats);
int pt_debug_denoiser_set_activation_frames(pt_denoiser* d, int layer, int frames, const float* h_in, size_t n_floats);
/* Convolution `conv` of the forward pass (execution order): info = {input layer, output layer (-1: the frame / rgb
 * buffer), second output layer, residual layer, upsampled layer, kernel size, stride, columns N, epilogue kind (0 affine,
 * 1 lateral upsample-add, 2 rgb head), split-K slices, tile rows, tile columns}. */
int pt_debug_denoiser_conv_info(pt_denoiser* d, int conv, int* n_convs, int info[12], char* name, size_t name_len);
/* Runs convolution `conv` alone on the workspace as it stands (synchronous); the rgb head writes [rows][cols][3] to d_rgb. */
int pt_debug_denoiser_run_conv(pt_denoiser* d, int conv, float* d_rgb);
/* Convolution `conv` of the plan of a group of `frames` frames, alone, on the first `frames` frames of the workspace as it
 * stands (synchronous; frames = 1 is the call above).  The rgb head writes channel n of pixel p of frame f to
 * d_out[f * frame_stride + p * ld + n]; every other convolution ignores d_out, ld and frame_stride.  Refused with PT_EINVAL,
 * nothing launched: frames outside 1 .. max_frames; the head without d_out, with ld < 3 or with frame_stride < width x
 * height x ld. */
int pt_debug_denoiser_run_conv_frames(pt_denoiser* d, int conv, float* d_out, int frames, int ld, size_t frame_stride);
/* The pre-processing of a group alone (the channel maxima, then the divisions and the stored copy "input"), synchronous:
 * `frames` frames of [rows][cols][14] floats, frame_stride floats apart; inplace != 0 also writes the normalised channels
 * 9-13 back.  Refused with PT_EINVAL, nothing launched: null d_frames, frames outside 1 .. max_frames, frame_stride <
 * width x height x 14. */
int pt_debug_denoiser_run_pre(pt_denoiser* d, float* d_frames, int frames, size_t frame_stride, int inplace);
/* Memory of the denoiser and of activation buffer `layer`, in bytes: info = {bytes per stored activation element (4, or 2
 * for a PT_DENOISE_F16 denoiser), the layer's offset into the workspace, the layer's size for ONE frame, the whole activation
 * workspace (all max_frames frames), the split-K partials (fp32 in both modes), the device weights}.  The activation and
 * set_activation calls above exchange float32 with the host in both modes (converted on the way; a half denoiser rounds
 * what is set to nearest even, saturating). */
int pt_debug_denoiser_memory(pt_denoiser* d, int layer, uint64_t info[6]);
/* The last enqueue (single or batch): *groups = frame groups it made, *launches = kernels it launched (0, 0 before any). */
int pt_debug_denoiser_last_enqueue(pt_denoiser* d, int* groups, int* launches);
/* Convolution `conv` of the plan of a group of n_frames frames (host arithmetic; any size inside the batch limits): info =
 * {rows M, tile rows, tile columns, split-K slices, 16-wide K chunks per slice, workgroups}.  n_frames = 1 is the single-frame
 * table that pt_debug_denoiser_conv_info reports. */
int pt_debug_denoiser_conv_plan(pt_denoiser* d, int n_frames, int conv, int info[6]);

/* Feature-guided filter (csrc/pt_filter.hip): the set-up and ONE iteration at `step` (1 .. 4096; the product runs 1, 2, 4, ...
 * in turn), fused with the re-modulation like a last iteration; arguments as pt_filter_enqueue.  Synchronous. */
int pt_debug_filter_step(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, int step);
/* on != 0: the iterations at steps 1 and 2 read an LDS tile (the workgroup's pixels and a clamped halo) instead of global
 * memory; the same bits (DENOISER.md, "Speed", has the measurement that decided the product's choice). */
int pt_debug_filter_tiled(pt_filter* f, int on);
/* The set-up and n_steps (0 .. 8) UNFUSED iterations at steps[k] (1 .. 4096 each), through the tile or direct loads as
 * pt_debug_filter_tiled says; then the current state {ill.rgb, var} and the guides {n.xyz, z}, {alb.rgb, dz}, each
 * [H][W][4] float32, are copied to d_state, d_guide0 and d_guide1.  The frame is only read.  d_frame, samples and d_counts as
 * pt_filter_enqueue.  Synchronous.  Both this call and pt_debug_filter_step honour pt_filter_set_spatial: the estimate runs
 * after the set-up, so with n_steps = 0 d_state holds the new var. */
int pt_debug_filter_state(pt_filter* f, const float* d_frame, int samples, const uint32_t* d_counts, const int* steps, int n_steps,
                          float* d_state, float* d_guide0, float* d_guide1);

/* Progressive sessions: set the session's sample count without rendering (the INT_MAX limit's test; the record is left as it
 * is, so the frames of later passes are meaningless).  samples < 0 is PT_EINVAL. */
int pt_debug_progressive_set_samples(pt_progressive* p, int64_t samples);
/* A copy of the session's record: PT_CHUNK_WORDS (26) words per tile pixel, [word][pixel] (synchronous).  Words (PT_REC_*,
 * csrc/pt_kernel.h): 0-8 the sums of colour, normal and albedo (x y z each), 9 the depth sum, 10 / 11 the Welford counts (the
 * colour's; the one the three first-hit accumulators share), 12-19 {mean, M2} of colour, normal, albedo, depth, 20-25 the
 * XORWOW generator d, v0 .. v4 (unused by philox sessions). */
int pt_debug_progressive_record(pt_progressive* p, uint32_t* host);
/* Adaptive sessions after their first pass: the next pass renders exactly the pixels whose byte in host_mask (one per tile
 * pixel) is non-zero, without the rule.  The set may only shrink: a pixel the last pass did not render is PT_EINVAL. */
int pt_debug_progressive_set_active(pt_progressive* p, const uint8_t* host_mask);
/* The selection in front of an adaptive pass (csrc/pt_adaptive.hip: classify, decide, scan, scatter) on a state the caller builds,
 * without a session or a renderer.  All pointers are HOST pointers; synchronous.  rec = [PT_CHUNK_WORDS (26)][tile_pixels] words
 * laid out like a session's record; mask, counts, list = tile_pixels entries each, words = {list length, maximum count}.  These
 * four go up to the device before the launch and come back afterwards whatever `peek` says, so a caller sees what a call left
 * alone and can chain calls by passing the output back in.  block_sums (may be NULL) receives the exclusive prefix of the
 * active pixels per 256-pixel block.  n = the count every active pixel holds, n_end > n = the count after the pass; mode 0 =
 * the rule on the pixels of mask bit 0, 1 = mask bit 0 as it is, 2 = every pixel; the rule is made from opts exactly as
 * pt_progressive_set_adaptive makes it (opts itself is not validated beyond the radius).  Every device array is an allocation
 * of its own, filled with a sentinel before the upload and followed by 64 guard words (the mask: 256 bytes): a guard that
 * changed is PT_EHIP with the array's name in the message. */
int pt_debug_adaptive_select(const uint32_t* rec, uint32_t tile_pixels, int width, int n, int n_end, int mode, int peek,
                             const pt_adaptive_opts* opts, uint8_t* mask, uint32_t* counts, uint32_t* list, uint32_t words[2],
                             uint32_t* block_sums);
/* The frame after an adaptive pass (adaptive_finalize_kernel): out = tile_pixels x 14 floats, [pixel][channel] or, planar != 0,
 * [channel][pixel], each pixel at counts[pixel] from rec.  Host pointers, synchronous, guarded like the call above. */
int pt_debug_adaptive_finalize(const uint32_t* rec, const uint32_t* counts, uint32_t tile_pixels, int planar, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PTCORE_LAB_H */
