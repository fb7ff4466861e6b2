/*
 * ptcore.h -- C ABI of libptcore.so: the MI355X (gfx950) implementation of the per-pixel
 * Monte-Carlo path-trace megakernel of trevor-m/cuda-pathtrace.
 *
 * This is the drop-in boundary.  The reference has no FFI layer; its boundary for this path
 * is header-level C++ (include/pathtrace.h, include/Renderer.h, include/OutputBuffer.h,
 * include/Scene.h).  Every entry point below names the reference interface it replaces
 * (file:line under the reference tree).  Plain pointers and sizes only; no C++ or torch
 * types.  The C++ look-alike classes that forward to these functions live in
 * cuda-pathtrace_amd/host/ (Renderer.h, OutputBuffer.h, Scene.h, Camera.h) and
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns PT_OK (0) or a negative PT_E* code; pt_last_error() returns a
 *     thread-local message for the last failure on the calling thread.  The reference's
 *     gpuErrchk (include/CudaErrorCheck.h:6-14) prints "GPUassert: <msg> <file> <line>"
 *     and exit()s; the C++ look-alikes reproduce that on a non-zero return.
 *   - "d_" pointers are device (HBM) addresses of the currently selected device; they may
 *     be foreign allocations (e.g. a torch CUDA tensor's data_ptr, as main.cu:104,134 does).
 *   - output layout is the reference's: float32 [row][col][14], channels
 *     0-2 colour RGB, 3-5 normal XYZ, 6-8 albedo RGB, 9 depth, 10 colourVar, 11 normalVar,
 *     12 albedoVar, 13 depthVar (src/pathtrace.cu:240-254).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point
 *     fails with PT_ENODEVICE / PT_EHIP.
 */
#ifndef PTCORE_H
#define PTCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 6

enum {
  PT_OK = 0,
  PT_EINVAL = -1,    /* bad argument                                         */
  PT_EHIP = -2,      /* a HIP runtime call failed (message has hipGetErrorString) */
  PT_ENODEVICE = -3, /* no HIP device visible                                */
  PT_ENOMEM = -4,    /* host allocation failed                               */
  PT_ELIMIT = -5,    /* scene does not fit the kernel's LDS staging budget   */
  PT_ECOMM = -6,     /* RCCL could not be loaded or a collective call failed (multi-GPU) */
  PT_ETIMEOUT = -7,  /* a multi-GPU frame did not complete in time; the exchange was aborted */
  PT_EKERNEL = -8    /* the kernel itself reported a failure (sample-chunk chain broken) for a frame that was  */
                     /*   ENQUEUED: that frame is incomplete -- the pixel blocks concerned were left untouched, */
                     /*   their generator state included (re-seed with pt_renderer_reset_rng / _set_rng_state   */
                     /*   to rejoin the reference's stream); sample chunking is off from then on.  A frame      */
                     /*   rendered with pt_renderer_render is completed by the call itself and returns PT_OK.   */
};

/* struct Sphere, include/Scene.h:7-14 -- same 40-byte layout, so a reference
 * `Sphere*` can be passed unchanged. */
typedef struct pt_sphere {
  float radius;
  float pos[3];
  float emission[3];
  float color[3];
} pt_sphere;

enum {
  PT_RNG_XORWOW = 0, /* cuRAND XORWOW, seed = pixel id (src/pathtrace.cu:265): reference parity */
  PT_RNG_PHILOX = 1  /* counter-based Philox4x32-10 keyed on (seed, frame); stateless           */
};

enum { PT_LAYOUT_INTERLEAVED = 0, PT_LAYOUT_PLANAR = 1 };

/* Options that the reference hard-codes or keeps in Renderer; zero-initialise then call
 * pt_renderer_opts_default(). */
typedef struct pt_renderer_opts {
  int32_t max_bounces;  /* MAX_BOUNCES, src/pathtrace.cu:7 (default 5)                     */
  int32_t rng_mode;     /* PT_RNG_*  (default PT_RNG_XORWOW)                               */
  uint64_t seed;        /* xorwow: added to the pixel id (0 = reference); philox: key      */
  int32_t row_begin;    /* rows [row_begin,row_end) of the width x height image are        */
  int32_t row_end;      /*   rendered by this renderer (multi-GPU row tiling); 0,0 = all   */
  int32_t persist_rng;  /* xorwow only: keep per-pixel generator state across Render()     */
                        /*   calls like Renderer::d_states (Renderer.h:17,37; pathtrace.cu:212,256); default 1 */
  int32_t variant;      /* kernel variant, all produce identical bits: -1 (default) = automatic    */
                        /*   (by scene size, tile size and generator), 0 = literal transcription,  */
                        /*   6, 8, 9, 10, 13, 14 see DESIGN.md section 3 (1-5, 7, 11, 12: libptcore_lab.so) */
  int32_t layout;       /* PT_LAYOUT_INTERLEAVED (default): the reference's [row][col][14] buffer  */
                        /*   (pathtrace.cu:240-254); PT_LAYOUT_PLANAR: [14][rows][width] of this   */
                        /*   renderer's tile -- same values, channel-first like a torch NCHW tensor */
  int32_t fast_math;    /* 0 (default): the bit-exact kernels.  1: the TOLERANCED fast mode -- same algorithm and */
                        /*   generator streams, FMA contraction allowed (nvcc's default for the reference), FP32-only   */
                        /*   cancellation-free intersectSphere, hardware rsq/sin/cos.  Distance from the reference's    */
                        /*   ORACLE at equal seeds, 256 x 256 (tests/test_fast_mode_gpu.py T5, profiles/r04/             */
                        /*   fast_vs_oracle.json): 1 spp -- albedo identical in >= 99.8 % of the pixels (measured:     */
                        /*   all), normals p99.9 6e-5 (L-inf 5e-4), depth p99.9 1e-5 relative; 64 spp -- colour beyond  */
                        /*   1e-4 in 1.6 % of the pixels (bound 3 %; median 0, L-inf 0.23: a ray that rounds onto       */
                        /*   another surface), normals 0.13 %, albedo 0.09 %; image means within 4 standard errors.      */
                        /*   NOT the north star's per-pixel L-inf 1e-4: only the exact kernels (bit-equal) meet that.   */
  int32_t chunks;       /* sample chunking (scheduling only, same bits): 0 (default) = automatic -- long frames of few   */
                        /*   workgroups split every pixel block's samples over several chained workgroups of one launch */
                        /*   (kernel map); 1 = never; 2..16 = that many chunks where the kernel supports it. */
                        /*   Costs scratch HBM (104 B per tile pixel) and hand-over traffic.  Env PT_CHUNKS overrides 0. */
  int32_t reserved;     /* must be 0 */
} pt_renderer_opts;

typedef struct pt_renderer pt_renderer; /* opaque; replaces class Renderer's private state, Renderer.h:10-20 */

/* ---- library / device -------------------------------------------------------------- */
int pt_abi_version(void);
/* 16 hex digits identifying the compiled sources + flags of this library (csrc/Makefile): measured
 * counters under profiles/ name the build they belong to. */
const char* pt_build_fingerprint(void);
const char* pt_last_error(void);
/* cudaSetDevice(cudaDevice), src/main.cu:86 */
int pt_set_device(int device);
int pt_device_count(int* count);
/* name + CU count of the selected device (for bench / logs) */
int pt_device_info(char* name, size_t name_len, int* compute_units, int* clock_khz);

/* ---- device memory: OutputBuffer / Scene allocations --------------------------------- */
/* cudaMalloc in OutputBuffer::AllocateGPU (OutputBuffer.h:73-74) and Scene() (Scene.h:36) */
int pt_malloc(void** d_ptr, size_t bytes);
/* cudaFree in OutputBuffer::FreeGPU (OutputBuffer.h:108-109) */
int pt_free(void* d_ptr);
/* cudaMemcpy H2D in Scene() (Scene.h:37) */
int pt_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
/* cudaMemcpy D2H in OutputBuffer::CopyFromGPU (OutputBuffer.h:49-50) */
int pt_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int pt_memset(void* d_ptr, int value, size_t bytes);
int pt_device_synchronize(void);

/* ---- Renderer ------------------------------------------------------------------------ */
void pt_renderer_opts_default(pt_renderer_opts* opts);

/* Renderer::Renderer(width, height, samplesPerPixel, numThreads), Renderer.h:23-46.
 * Allocates the per-pixel generator state and runs setup_random (pathtrace.cu:259-266)
 * when rng_mode == PT_RNG_XORWOW && persist_rng.  threads_per_block is accepted for CLI
 * compatibility (main.cu:21,34) and ignored: the kernel picks its own workgroup shape.
 * opts may be NULL (= defaults). */
int pt_renderer_create(int width, int height, int samples_per_pixel, int threads_per_block,
                       const pt_renderer_opts* opts, pt_renderer** out);

/* Renderer::~Renderer(), Renderer.h:48-53 */
int pt_renderer_destroy(pt_renderer* r);

/* Renderer::Render(OutputBuffer d_buffer, const Scene& d_scene, const Camera& camera),
 * Renderer.h:55-76.  d_out points at the first float of row `row_begin` (for a full-frame
 * renderer: the buffer base).  basis = the 4 corner directions of
 * Camera::getEyeRayBasis (Camera.h:125-149), eye = camera.Position.  Synchronous like the
 * reference (returns after the stop event), *ms_out = kernel-only milliseconds from a
 * hipEvent pair (Renderer.h:63-75).  ms_out may be NULL.  (A frame whose sample-chunk chain broke -- never observed; see
 * PT_EKERNEL -- is repaired in place by a second launch: *ms_out then holds both launches INCLUDING the wait limit, default
 * 4 s, a line goes to stderr, pt_last_error() carries the same text and pt_renderer_check counts the frame.) */
int pt_renderer_render(pt_renderer* r, float* d_out, const pt_sphere* d_spheres, int n_spheres,
                       const float basis[12], const float eye[3], float* ms_out);

/* Same launch without host synchronisation, on the caller's HIP stream (hipStream_t passed
 * as void*; NULL = the default stream).  Used by bench.py and the multi-GPU driver so the
 * kernel overlaps with the caller's copies/collectives and can be timed with the caller's
 * events.  The camera (60 B) travels as kernel arguments: no H2D copy, no allocation.
 * One renderer's launches always execute in submission order: the renderer owns per-frame device
 * scratch (generator state, grid tables), so a launch on a different stream than the previous one
 * first waits (hipStreamWaitEvent) for that previous launch.  Frames that should overlap need
 * separate renderers. */
int pt_renderer_enqueue(pt_renderer* r, float* d_out, const pt_sphere* d_spheres, int n_spheres,
                        const float basis[12], const float eye[3], void* hip_stream);

/* n_frames frames with KNOWN cameras: what n_frames calls of pt_renderer_enqueue(r, d_out + f * out_stride_floats, ..., bases +
 * 12 f, eyes + 3 f, stream) do -- the body of the reference's frame loop (src/main.cu:146-177, `renderer.Render(...)` per
 * iteration) for a scripted fly-through or a pose sweep (collect_data.py) -- same frames, same persisted generator state
 * afterwards (src/pathtrace.cu:212,256), bit for bit.  For the reference's scene in the reference configuration (9 spheres, 5 or
 * 8 bounces, interleaved layout: the interactive shape, whose single frame is one round of waves -- all ramp and tail) the frames
 * go out as ONE launch per 32: a workgroup keeps its pixels for the whole batch and loops over the frames, the generator staying
 * in its registers from frame to frame (the counter-based one is re-keyed per frame) -- no state traffic, one ramp and one tail
 * per batch.  Elsewhere it IS the loop of single enqueues -- also for an XORWOW renderer created with persist_rng = 0, whose
 * every frame starts from the seeded stream (a generator kept in registers would carry on instead); the counter-based
 * generator is keyed by the frame counter alone and is batched with or without persist_rng.
 * d_vertices != NULL: frame f also writes its display vertices to d_vertices + f * vtx_stride_floats (pt_renderer_set_display
 * for the batch).  Frames that would share a buffer (out_stride_floats below one tile, a set_display buffer without
 * d_vertices) are rendered one by one.  bases / eyes are host arrays, read before the call returns. */
int pt_renderer_enqueue_frames(pt_renderer* r, int n_frames, float* d_out, size_t out_stride_floats, float* d_vertices,
                               size_t vtx_stride_floats, const pt_sphere* d_spheres, int n_spheres, const float* bases,
                               const float* eyes, void* hip_stream);

/* Status of the frames enqueued so far (wait != 0: block until the last one's status word has arrived): PT_OK, or
 * PT_EKERNEL once for a frame whose sample-chunk chain broke (see PT_EKERNEL; the next pt_renderer_enqueue /
 * pt_renderer_render on the renderer would report it otherwise).  Call it after synchronising on the stream and
 * before pt_renderer_destroy, which reports nothing.  *repaired_frames (may be NULL) receives the number of frames
 * whose broken chain pt_renderer_render has repaired in place since the renderer was created (normally 0). */
int pt_renderer_check(pt_renderer* r, int wait, uint32_t* repaired_frames);

/* Renderer::Render + Denoiser::Denoise in ONE kernel (the body of the reference's interactive loop, src/main.cu:148,175):
 * from now on every frame of this renderer also writes the display vertices denoise_kernel (src/denoise.cu:9-29) derives
 * from it -- (col, width - row, RGBA8 {r,g,b,1} packed in a float) per pixel -- straight from the registers that hold the
 * pixel's colour: no second launch, no 12 B per pixel read back.  d_vertices: device float [rows of this renderer][width][3],
 * first vertex = first pixel of row_begin (like d_out); NULL switches it off.  Bit-identical to pt_display_pack(frame). */
int pt_renderer_set_display(pt_renderer* r, float* d_vertices);

/* Frame counter used by the philox key; incremented by every render/enqueue. */
int pt_renderer_set_frame(pt_renderer* r, uint32_t frame);
/* Re-run setup_random (pathtrace.cu:259-266): generator state as after construction. */
int pt_renderer_reset_rng(pt_renderer* r);
/* Copy the xorwow state ({d,v0..v4} = 6 x uint32 per tile pixel) to / from the host. */
int pt_renderer_get_rng_state(pt_renderer* r, uint32_t* h_state, size_t n_words);
int pt_renderer_set_rng_state(pt_renderer* r, const uint32_t* h_state, size_t n_words);
/* Static facts about the compiled kernel the renderer will launch. */
typedef struct pt_kernel_info {
  int32_t block_threads;
  int32_t grid_blocks;
  int32_t lds_bytes;
  int32_t num_vgprs;    /* from hipFuncGetAttributes */
  int32_t reserved0;    /* always 0 (was num_sgprs up to ABI 5: hipFuncGetAttributes does not report scalar registers) */
  int32_t scratch_bytes;
  int32_t max_spheres;  /* LDS staging limit for this variant (2^26 where larger scenes are not staged) */
  int32_t variant;      /* the variant the next launch will use (resolves the automatic choice) */
} pt_kernel_info;
int pt_renderer_kernel_info(pt_renderer* r, int n_spheres, pt_kernel_info* info);

/* ---- sphere materials (opt-in; csrc/pt_materials.hip, EXACTNESS.md A.22) --------------------- */
/* The reference renders diffuse surfaces only.  A material table gives every sphere one of four kinds; a renderer without a
 * table is exactly what it was.  EXACT code: the frame equals tests/materials_model.py, the definition in NumPy float32, bit
 * for bit, and with an all-diffuse table it equals the oracle's frame.  Every kind takes the two generator draws of a bounce,
 * so both generators serve as they are. */
enum {
  PT_MATERIAL_DIFFUSE = 0, /* the reference's bounce; param 0                                                    */
  PT_MATERIAL_MIRROR = 1,  /* a perfect mirror; param 0                                                          */
  PT_MATERIAL_GLOSSY = 2,  /* the mirror direction blended towards the diffuse one by param = roughness, 0 < rho < 1 */
  PT_MATERIAL_GLASS = 3    /* smallpt's dielectric with Schlick's Fresnel term; param = index of refraction, 1 < eta <= 4 */
};
typedef struct pt_material {
  int32_t kind; /* PT_MATERIAL_* */
  float param;
} pt_material;
#define PT_MATERIALS_MAX_SPHERES 64 /* a scene with a table is staged whole: more spheres are PT_ELIMIT */
#define PT_VARIANT_MATERIALS 101    /* pt_kernel_info.variant while a table is set (a pseudo-variant like the fast mode's 100: no
                                     * row of the variant table, no value of pt_renderer_opts.variant) */
/* The host checks of pt_renderer_set_materials alone (no device, no renderer): PT_EINVAL naming the entry for a null table,
 * n < 1, a kind outside 0..3, a param that is not finite or outside its kind's range, a non-zero param for DIFFUSE or MIRROR;
 * PT_ELIMIT for n > PT_MATERIALS_MAX_SPHERES. */
int pt_material_check(const pt_material* table, int n);
/* One material per sphere, in sphere order (host array, copied to the device before the call returns; it synchronises the
 * device first, so no frame in flight reads a table that is being replaced).  While a table is set EVERY render / enqueue of the
 * renderer runs the materials kernel -- an all-diffuse table too: no silent fallback -- and pt_renderer_kernel_info reports
 * PT_VARIANT_MATERIALS; a render whose n_spheres differs from n is PT_EINVAL and launches nothing, pt_renderer_enqueue_frames is
 * the loop of single enqueues, and pt_progressive_create / a session's passes are refused.  (NULL, 0) clears the table: the
 * renderer runs the ordinary kernels again, bit for bit as before.  Refused (PT_EINVAL, before a device is touched): whatever
 * pt_material_check refuses, a fast_math renderer, a renderer with an explicit kernel variant.  Both output layouts and the
 * display vertices of pt_renderer_set_display are supported.  pt_mgpu has no materials. */
int pt_renderer_set_materials(pt_renderer* r, const pt_material* host_table, int n);

/* ---- direct light sampling (opt-in; csrc/pt_materials.hip, EXACTNESS.md A.23) ----------------- */
/* Departs from src/pathtrace.cu's emission-only accumulation (:171-174: a path gains light only when a bounce happens to land
 * on an emitter).  With the option on, every DIFFUSE hit but the last bounce's also draws one direction inside the cone each
 * emitting sphere subtends, traces a shadow ray, and adds that light's direct contribution; the next hit leaves out the
 * emission of the lights so accounted for.  The frame's expectation is that of the frame without the option at the same
 * max_bounces: the noise changes, not the picture.  EXACT code: the frame equals tests/lights_model.py bit for bit.
 * on != 0: every render / enqueue runs the materials kernel's light-sampling build and pt_renderer_kernel_info reports
 * PT_VARIANT_MATERIALS_LIGHTS -- with the renderer's material table, or, without one, with every sphere DIFFUSE (a scene above
 * PT_MATERIALS_MAX_SPHERES is then PT_ELIMIT and nothing is launched).  on == 0: the renderer is exactly what it was
 * (PT_VARIANT_MATERIALS with a table, the ordinary kernels without).  The order of pt_renderer_set_materials and this call does
 * not matter.  Refused (PT_EINVAL): a NULL renderer, a fast_math renderer, a renderer with an explicit kernel variant; while it
 * is on, pt_progressive_create, a session's passes and pt_renderer_enqueue_frames are refused.  pt_mgpu has no light sampling. */
#define PT_VARIANT_MATERIALS_LIGHTS 102 /* a pseudo-variant like PT_VARIANT_MATERIALS */
int pt_renderer_set_light_sampling(pt_renderer* r, int on);

/* ---- sky and sun (opt-in; csrc/pt_materials.hip, EXACTNESS.md A.24) --------------------------- */
/* Departs from src/pathtrace.cu:157-161, where a ray that leaves the scene returns nothing.  With a sky set, an escaping path
 * takes the radiance of its direction u (world up is +y): horizon + (zenith - horizon) * u.y where u.y >= 0, ground elsewhere,
 * plus sun_radiance where dot(u, sun_dir) >= sun_cos.  A primary ray's sky is clamped to [0, 1] per component like an emitter
 * seen directly (:171-172); the first-hit features of such a sample stay zero; every sample, escaped or not, enters the colour
 * variance.  With pt_renderer_set_light_sampling on, the sun is the last light of A.23's list: one direction inside its cone
 * and one shadow ray per DIFFUSE hit but the last bounce's, lit iff the ray leaves the scene, and the escape that follows takes
 * the gradient without the disc.  EXACT code: the frame equals tests/sky_model.py bit for bit. */
typedef struct pt_sky {
  float zenith[3];       /* radiance straight up */
  float horizon[3];      /* radiance at the horizon */
  float ground[3];       /* radiance of every direction with u.y < 0 */
  float sun_dir[3];      /* direction TOWARDS the sun, any length: normalised on the host in float32 */
  float sun_cos;         /* cosine of the sun's angular radius */
  float sun_radiance[3]; /* radiance of the disc; all zero: no sun, and sun_dir / sun_cos are not read */
} pt_sky;
#define PT_VARIANT_MATERIALS_SKY 103        /* pseudo-variants like PT_VARIANT_MATERIALS: a sky is set, ... */
#define PT_VARIANT_MATERIALS_LIGHTS_SKY 104 /* ... and direct light sampling is on */
/* The host checks of pt_renderer_set_sky alone (no device, no renderer): PT_EINVAL naming the field for a NULL pointer; a
 * radiance component (zenith, horizon, ground, sun_radiance) that is not finite or is negative; with a sun (a sun_radiance
 * component > 0) a sun_dir that is not finite or of zero length, a sun_cos outside [0, 1) or with 1 - sun_cos < 2^-20. */
int pt_sky_check(const pt_sky* sky);
/* Copies the description; NULL clears it and the renderer is exactly what it was.  While a sky is set EVERY render / enqueue
 * runs a SKY build of the materials kernel -- with the renderer's material table, or, without one, with every sphere DIFFUSE
 * (a scene above PT_MATERIALS_MAX_SPHERES is then PT_ELIMIT and nothing is launched) -- and pt_renderer_kernel_info reports
 * PT_VARIANT_MATERIALS_SKY, or PT_VARIANT_MATERIALS_LIGHTS_SKY with light sampling on.  The order of pt_renderer_set_materials,
 * pt_renderer_set_light_sampling and this call does not matter.  Refused (PT_EINVAL): whatever pt_sky_check refuses, a NULL
 * renderer, a fast_math renderer, a renderer with an explicit kernel variant; while a sky is set, pt_progressive_create and a
 * session's passes are refused, and pt_renderer_enqueue_frames is the loop of single enqueues (refused with light sampling
 * on, as without a sky).  pt_mgpu has no sky. */
int pt_renderer_set_sky(pt_renderer* r, const pt_sky* sky);

/* ---- one frame over several GPUs of one node ------------------------------------------------- */
/* The reference selects ONE device per process (cudaSetDevice(cudaDevice), src/main.cu:86) and its
 * Renderer covers the whole image with one launch (Renderer.h:29-33,69).  pt_mgpu_* is the same
 * Renderer boundary over N devices: the image is cut into N contiguous row blocks (pixels are
 * independent and every generator is keyed on the global pixel id, pathtrace.cu:206,265, so the
 * result does not depend on the cut), one host thread per device renders its block, and ONE
 * exchange step per frame places the blocks in the caller's frame on devices[0]: grouped RCCL
 * ncclRecv x (N-1) on the root straight into the frame at the tile offsets | one ncclSend per peer.
 * Single process, no launcher; RCCL is dlopen'ed on first use. */
enum {
  PT_GATHER_AUTO = 0,      /* RCCL between distinct devices, peer copies if ranks share a device   */
  PT_GATHER_RCCL = 1,      /* ncclGroupStart{ncclRecv x (N-1) | ncclSend}ncclGroupEnd over xGMI     */
  PT_GATHER_PEER_COPY = 2  /* hipMemcpyPeerAsync of each tile on its own stream (SDMA over xGMI)    */
};
typedef struct pt_mgpu_opts {
  int32_t gather;          /* PT_GATHER_*                                                          */
  int32_t force_exchange;  /* 1: even the root's tile is rendered into a tile buffer and travels   */
                           /*    through the exchange step (self send/recv): exercises the whole   */
                           /*    multi-GPU path on a single-GPU machine.  Env PT_FORCE_MGPU=1.      */
  int32_t timeout_ms;      /* a frame not complete after this long fails with PT_ETIMEOUT and the  */
                           /*    communicator is aborted (0 = wait forever).  Env PT_MGPU_TIMEOUT_MS, default 60000 */
  int32_t bands;           /* row bands a rank's tile is rendered in: band b's transfer overlaps band b+1's   */
                           /*    kernel, only the last band's is exposed.  0 = automatic (bands of at least    */
                           /*    eight one-lane waves per SIMD, at most 8; 1 when no tile crosses a link), 1..64. */
                           /*    Env PT_MGPU_BANDS.  Same bits whatever the value.                               */
} pt_mgpu_opts;
typedef struct pt_mgpu pt_mgpu; /* opaque */

/* Defaults, with the environment overrides PT_FORCE_MGPU, PT_MGPU_TIMEOUT_MS, PT_MGPU_GATHER=rccl|copy, PT_MGPU_BANDS. */
void pt_mgpu_opts_default(pt_mgpu_opts* opts);
/* Renderer::Renderer over n_gpus devices (devices == NULL: 0..n_gpus-1; devices[0] is the root that
 * owns the caller's frame and scene).  opts as for pt_renderer_create, with row_begin = row_end = 0;
 * mopts may be NULL.  Creates per device: a renderer for its row block (generator state included),
 * a stream, a tile buffer; and one RCCL communicator over all of them (ncclCommInitAll). */
int pt_mgpu_create(int n_gpus, const int* devices, int width, int height, int samples_per_pixel,
                   int threads_per_block, const pt_renderer_opts* opts, const pt_mgpu_opts* mopts,
                   pt_mgpu** out);
int pt_mgpu_destroy(pt_mgpu* m);
/* Error behaviour of pt_mgpu_render: a rank that cannot render still posts its part of the exchange (nobody waits for
 * a tile that never comes) and the call reports the first failure.  After PT_ETIMEOUT, or any failure in which a rank lost
 * its communicator (ncclCommAbort), the object is dead: every later pt_mgpu_render returns PT_ECOMM and pt_mgpu_destroy is
 * the only call it still accepts.  Other failures (PT_EINVAL, PT_ELIMIT, PT_EHIP from a rank's render) leave it usable. */
/* Renderer::Render (Renderer.h:55-76) for the whole frame: d_out ([height][width][14]) and
 * d_spheres live on devices[0] and must be complete (the call does not order itself after the
 * caller's streams); the scene is replicated to the other devices by peer copies (360 B .. 40 KB).
 * Synchronous: returns when the frame is assembled.  *ms_out = end-to-end wall milliseconds
 * (render + exchange); per-tile kernel times: pt_mgpu_tile. */
int pt_mgpu_render(pt_mgpu* m, float* d_out, const pt_sphere* d_spheres, int n_spheres,
                   const float basis[12], const float eye[3], float* ms_out);
/* Row block, device and last kernel time of a rank (any out pointer may be NULL). */
int pt_mgpu_tile(pt_mgpu* m, int rank, int* device, int* row_begin, int* row_end, float* kernel_ms);
/* Timing of the last pt_mgpu_render (any out pointer may be NULL): bands per tile, the longest rank's render time (first
 * launch to last band done, hipEvent pair) and what the exchange added on top of it (end-to-end wall time minus that). */
int pt_mgpu_frame_stats(pt_mgpu* m, int* bands, float* render_ms, float* exposed_ms);
/* Name of the exchange backend in use (for logs / bench). */
int pt_mgpu_backend(pt_mgpu* m, char* name, size_t name_len);

/* ---- display packing ------------------------------------------------------------------- */
/* Denoiser::Denoise -> denoise_kernel (include/Denoiser.h:29-52, src/denoise.cu:9-29): despite the
 * name, the reference's "denoiser" only prepares the frame for its point-sprite display: colour
 * clamped to [0,1] and packed as RGBA8 {r,g,b,1} into ONE float, written with the pixel's screen
 * position as the vertex triple (col, width - row, packed) into d_vertices[row][col][3].  The
 * OpenGL buffer the reference maps (GLPixelBuffer) is replaced by a plain device pointer.
 * Asynchronous on hip_stream (NULL = default stream). */
int pt_display_pack(const float* d_buffer, int width, int height, float* d_vertices, void* hip_stream);

/* ---- denoising network ---------------------------------------------------------------- */
/* The reference's `-d` step (src/main.cu:92-122,146-152): after every Render() the interactive loop runs DenoiseCNN
 * (denoise_cnn/model.py) on the frame tensor in place through train.py:test() (pre-processing train.py:48-55, eval-mode
 * forward, modify_tensor main.cu:106 writes the RGB result into channels 0-2).  Here: fp32 MFMA inference in HIP for a
 * fixed width x height (DENOISER.md).  Result in place: channels 0-2 = clamp(net, 0, 1), 3-8 as rendered, 9-13 normalised
 * (divided by 0.00316 + the channel's max, that sum formed in double as torch 0.2/0.3's Python-float max did).
 *
 * Weights: the reference ships none; a state_dict trained by its train.py (its parameter names, e.g. block1.res_conv.weight,
 * block1.res_bn.running_var, lat_0.bias, backwards_10.weight, rgb_conv.weight; num_batches_tracked dropped) is written as a
 * PTDN image by cuda-pathtrace_amd/denoise_weights.py.  Layout, little-endian, no padding or alignment:
 *   char magic[4] = "PTDN"; uint32 version = 1; uint32 n_tensors;
 *   n_tensors x { uint32 name_len; char name[name_len] (UTF-8, no NUL); uint32 ndim; uint32 dims[ndim];
 *                 float32 data[prod(dims)] (row-major, torch's order) }
 * A file with a missing, unexpected, repeated or wrongly shaped tensor, a truncation or trailing bytes is rejected with
 * PT_EINVAL and a message naming the key.  Host only; needs no device. */
typedef struct pt_denoiser pt_denoiser; /* opaque: the network's weights + the activation workspace of one frame size */
int pt_denoiser_weights_check(const void* blob, size_t bytes);
/* DenoiseCNN() + load_pretrained (the model train.py loads for main.cu:92-102) for width x height frames (H = rows):
 * uploads the weights (re-laid out for the GEMMs, batch norm folded) and allocates the workspace on the current device. */
int pt_denoiser_create(int width, int height, const void* blob, size_t bytes, pt_denoiser** out);
int pt_denoiser_create_from_file(int width, int height, const char* path, pt_denoiser** out);
int pt_denoiser_destroy(pt_denoiser* d);
/* Half precision (opt-in; pt_denoiser_create is PT_DENOISE_F32 and unchanged).  PT_DENOISE_F16 runs the same network with
 * fp16 operands and storage and fp32 accumulation (v_mfma_f32_32x32x16_f16): the convolution weights are rounded once (to
 * nearest even) at create time, every stored activation -- the workspace copy of the pre-processed frame included -- is
 * fp16, and every epilogue (bias, ReLU, batch norm, residual, upsample + lateral, albedo multiply and clamp) is computed in
 * fp32 and rounded once on its store.  Every such store SATURATES to +-65504 instead of producing an infinity (what a NaN
 * becomes is unspecified, as it is for the fp32 mode's ReLU).  What lands in the caller's frame is fp32 as before: channels
 * 0-2 the clamped result, 3-8 untouched, 9-13 divided in fp32 exactly as in the fp32 mode (bit for bit).  Bias and the folded
 * batch norm stay fp32.  Tolerance contract (like fast_math's: tests/test_denoiser_half_gpu.py holds it): against the
 * float64 network on the same frame, the [0, 1] output's error is within 2 x rms + 1e-5 and 3 x max + 1e-4 of the error of
 * the float64 network with the same roundings inserted (tests/denoise_half_model.py); that model's own error on 64 x 64
 * frames with seeded random weights is 0.8e-3 .. 3.1e-3 max, 1.4e-4 .. 5.2e-4 rms (half an 8-bit display step is 2.0e-3).
 * The values measured on the GPU are in DENOISER.md, "Half precision".  Runs are deterministic and batches keep the
 * bit-for-bit contract of pt_denoiser_enqueue_frames within the mode.  The workspace is half the fp32 mode's bytes.
 * opts: precision = PT_DENOISE_F32 or PT_DENOISE_F16; max_frames >= 1 = pt_denoiser_reserve_frames(max_frames) at create
 * time; reserved words must be 0.  Anything else, or (PT_DENOISE_F16) a convolution weight beyond +-65504, is PT_EINVAL
 * naming the argument or the tensor, before a device is touched. */
enum { PT_DENOISE_F32 = 0, PT_DENOISE_F16 = 1 };
typedef struct pt_denoiser_opts {
  int32_t precision;  /* PT_DENOISE_*                      */
  int32_t max_frames; /* frames per group, >= 1            */
  int32_t reserved[6]; /* must be 0                        */
} pt_denoiser_opts;
int pt_denoiser_create_opts(int width, int height, const void* blob, size_t bytes, const pt_denoiser_opts* opts, pt_denoiser** out);
int pt_denoiser_create_opts_from_file(int width, int height, const char* path, const pt_denoiser_opts* opts, pt_denoiser** out);
int pt_denoiser_precision(const pt_denoiser* d, int* out); /* *out = PT_DENOISE_F32 or PT_DENOISE_F16 */
/* train.py:test(model, boost_tensor) + modify_tensor (main.cu:106,150-152) on the device frame d_frame ([height][width][14]),
 * asynchronous on hip_stream (NULL = default stream).  d_rgb == NULL: the reference's in-place semantics.  d_rgb != NULL:
 * the result goes to d_rgb ([height][width][3]) and d_frame is left byte for byte untouched.  One denoiser's enqueues share
 * its workspace: do not run two of them concurrently on different streams. */
int pt_denoiser_enqueue(pt_denoiser* d, float* d_frame, float* d_rgb, void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around the
 * network, like Renderer::Render (Renderer.h:63-75). */
int pt_denoiser_denoise(pt_denoiser* d, float* d_frame, float* d_rgb, float* ms_out);
/* Batches.  pt_denoiser_enqueue_frames(d, n, d_frames, frame_stride, d_rgb, rgb_stride, s) does, bit for bit, what
 *   for f in 0 .. n-1: pt_denoiser_enqueue(d, d_frames + f * frame_stride, d_rgb ? d_rgb + f * rgb_stride : NULL, s)
 * does: every frame is pre-processed with its own channel maxima, in place (d_rgb == NULL) or out of place (frames untouched).
 * Frames go through the network in groups of up to max_frames (1 unless reserved), each group in the launches of ONE frame:
 * its frames are rows of the same GEMMs, with each layer's split of K kept from the single-frame plan (DENOISER.md, "Batches").
 * Strides are in floats: frame_stride >= width x height x 14, rgb_stride >= width x height x 3 when d_rgb is given, so the
 * strided output of pt_renderer_enqueue_frames can be passed straight in.  n_frames >= 1; any other value, a null denoiser
 * or null frames is PT_EINVAL naming the argument, and nothing is launched.  Asynchronous on hip_stream (NULL = default).
 * pt_denoiser_reserve_frames grows the workspace (about 114 MB per 512x512 frame plus the split-K partials) for groups of up
 * to max_frames frames; max_frames <= the current value is a no-op.  Limits: max_frames <= 65535 and max_frames x width x
 * height <= 2^26 pixels (PT_EINVAL beyond).  It synchronises the device before freeing the old workspace; on failure
 * (PT_EHIP) the old workspace stays in use. */
int pt_denoiser_reserve_frames(pt_denoiser* d, int max_frames);
int pt_denoiser_enqueue_frames(pt_denoiser* d, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                               size_t rgb_stride_floats, void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = device-event milliseconds around all the groups. */
int pt_denoiser_denoise_frames(pt_denoiser* d, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                               size_t rgb_stride_floats, float* ms_out);

/* ---- feature-guided filter: the weights-free denoiser --------------------------------------- */
/* No counterpart in the reference, whose only denoiser is the CNN above and which ships no weights for it.  The frame itself
 * carries what a feature-guided filter needs (src/pathtrace.cu:240-254: mean colour, normal, albedo, depth and the sample
 * variance of each), so pt_filter_* turns a 2 .. 16 spp frame into a usable picture without outside data: an edge-avoiding
 * a-trous wavelet filter on albedo-demodulated colour, its luminance stop scaled by the pixel's own variance (the spatial
 * stage of SVGF), its stops on normal, albedo and depth taken from the frame's channels.  TOLERANCED code like fast_math:
 * DENOISER.md, "Feature-guided filter", states the definition and the measured distance from its float64 restatement
 * (tests/filter_model.py).  Deterministic: no atomics, two runs give the same bits.
 *   With EPS = 0.00316f (train.py:48-55), lum(c) = 0.2126 c.x + 0.7152 c.y + 0.0722 c.z and a = EPS + albedo per channel:
 *   set-up    ill = colour / a;  n = the pixel's count (d_counts) or `samples`;  var = ch10 / n / lum(a)^2 when n >= 2, else
 *             lum(ill)^2;  dz = 0.5 max(|z[y][x+1] - z[y][x-1]|, |z[y+1][x] - z[y-1][x]|), indices clamped.
 *   iteration i = 0 .. iterations-1, step s = 2^i:  g = the 3 x 3 (1/4, 1/2, 1/4)^2 blur of var (replicated edges),
 *             sd = sqrt(max(g, 0)), L = lum(ill); over the 25 taps q = p + s (i, j), i, j in -2 .. 2 that lie inside the frame,
 *             h = k[i] k[j] with k = (1/16, 1/4, 3/8, 1/4, 1/16), d = s sqrt(i^2 + j^2):
 *               e = |n_q - n_p|^2 / sigma_n^2 + |alb_q - alb_p|^2 / sigma_a^2
 *                 + |z_q - z_p| / (sigma_z dz_p d + 1e-3 |z_p| + 1e-20) + |L_q - L_p| / (sigma_l sd_p + 0.01 |L_p| + 1e-4)
 *               w = h exp(-e);   ill' = sum(w ill_q) / sum(w);   var' = sum(w^2 var_q) / sum(w)^2
 *   result    ill (EPS + albedo): unclamped radiance.  In place it replaces channels 0-2 and channels 3-13 are not written; out
 *             of place it goes to d_rgb ([height][width][3]) and the frame is left byte for byte untouched.
 * Limits: the colour variance skips escaped paths (pathtrace.cu:157-161), so in open scenes channel 10 rests on fewer than n
 * samples, which the filter ignores; and the variance transfer above is the definition, not an identity, for a coloured albedo.
 * Workspace: 64 bytes per pixel and frame of a group (pt_filter_workspace_bytes). */
typedef struct pt_filter_opts {
  int32_t iterations;  /* 1 .. 8 (default 5): steps 1, 2, 4, ...                          */
  float sigma_l;       /* luminance stop, in standard deviations (default 4.0)            */
  float sigma_n;       /* normal stop (default 0.35)                                      */
  float sigma_a;       /* albedo stop (default 0.1)                                       */
  float sigma_z;       /* depth stop, in screen-space depth slopes (default 1.0)          */
  int32_t max_frames;  /* frames per group, >= 1 (default 1)                              */
  int32_t reserved[2]; /* must be 0                                                       */
} pt_filter_opts;
typedef struct pt_filter pt_filter; /* opaque: the options + the workspace of one frame size */
void pt_filter_opts_default(pt_filter_opts* opts);
/* opts may be NULL (= defaults).  Every option is validated BEFORE a device is touched: iterations outside 1 .. 8, a sigma that
 * is not finite and > 0, max_frames < 1 (or beyond the limits of pt_filter_reserve_frames), a non-zero reserved word or a
 * width / height outside 1 .. 4096 x 4096 pixels (a side at most 16384) is PT_EINVAL naming the argument.  Allocates the workspace on the current device. */
int pt_filter_create(int width, int height, const pt_filter_opts* opts, pt_filter** out);
int pt_filter_destroy(pt_filter* f);
/* Grows the workspace for groups of up to max_frames frames; max_frames <= the current value is a no-op.  Limits: max_frames
 * <= 65535 and max_frames x width x height <= 2^26 pixels (PT_EINVAL beyond).  It synchronises the device before freeing the
 * old workspace; on failure (PT_EHIP) the old workspace stays in use. */
int pt_filter_reserve_frames(pt_filter* f, int max_frames);
int pt_filter_workspace_bytes(const pt_filter* f, uint64_t* bytes);
/* Filters the device frame d_frame ([height][width][14]), asynchronous on hip_stream (NULL = default stream).  d_rgb == NULL:
 * in place; d_rgb != NULL: out of place.  samples >= 1 is the frame's uniform count; with d_counts != NULL (uint32
 * [height][width], what pt_progressive_counts writes) every pixel uses its own count and samples is ignored.  The iterations
 * never read the caller's frame (the last one writes it), so in-place use is safe.  One filter's enqueues share its workspace:
 * do not run two of them concurrently on different streams.  A null filter or frame, or samples < 1 without a count image, is
 * PT_EINVAL and nothing is launched. */
int pt_filter_enqueue(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around the
 * filter, like pt_denoiser_denoise. */
int pt_filter_run(pt_filter* f, float* d_frame, float* d_rgb, int samples, const uint32_t* d_counts, float* ms_out);
/* Batches, with the contract and limits of pt_denoiser_enqueue_frames: bit for bit what
 *   for k in 0 .. n-1: pt_filter_enqueue(f, d_frames + k * frame_stride, d_rgb ? d_rgb + k * rgb_stride : NULL, samples, NULL, s)
 * does.  Frames go through in groups of up to max_frames, each group in the launches of ONE frame (1 + iterations).  Strides are
 * in floats and may leave gaps (frame_stride >= width x height x 14, rgb_stride >= width x height x 3 when d_rgb is given), so
 * the strided output of pt_renderer_enqueue_frames can be passed straight in.  There is no count image in the batch form.
 * n_frames < 1, a stride too small, samples < 1, a null filter or null frames is PT_EINVAL naming the argument, and nothing is
 * launched. */
int pt_filter_enqueue_frames(pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                             size_t rgb_stride_floats, int samples, void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = device-event milliseconds around all the groups. */
int pt_filter_run_frames(pt_filter* f, int n_frames, float* d_frames, size_t frame_stride_floats, float* d_rgb,
                         size_t rgb_stride_floats, int samples, float* ms_out);

/* -- spatial variance estimate: the variance of a pixel with few samples, from its neighbours (DENOISER.md, "Spatial variance
 * estimate") --
 * At 1 .. 4 samples the pixel's own variance above says little: most paths of a closed scene return 0 until one finds the
 * light, so many pixels report a variance of exactly 0 and stop the luminance stop dead, and n = 1 has no variance at all.
 * With the mode on, ONE more launch between the set-up and the first iteration gives every pixel p whose integer count n_p (its
 * entry of d_counts, else `samples`) is below `below` the spread of its neighbours' means on the same surface, which estimates
 * the same quantity var holds (SVGF does this where a pixel's history is short).  With L = lum(ill), over the taps q = p + (i, j),
 * |i|, |j| <= radius, that lie inside the frame (restated in tests/filter_spatial_model.py):
 *     e = |n_q - n_p|^2 / sigma_n^2 + |alb_q - alb_p|^2 / sigma_a^2 + |z_q - z_p| / (sigma_z dz_p sqrt(i^2 + j^2) + 1e-3 |z_p| + 1e-20)
 *     w = exp(-e) (the centre: 1);   m = sum(w L_q) / sum(w);   v = sum(w (L_q - m)^2) / sum(w);   var_p = fmax(var_p, v)
 * The sigmas are the filter's own; there is no luminance term.  v is taken in two passes, centred, on L_q - L_p (the same v; a
 * window of equal luminances gives exactly 0), and fmax leaves var_p alone when v is NaN.  A pixel with n_p >= below keeps its var bit for bit, and the iterations are unchanged.  TOLERANCED code like the
 * iterations in e and w; the two moment sums are rounded operation by operation, row by row through the window.
 * Off (the default), every call keeps its bits and its launches; on, a call whose pixels cannot qualify (no count image and
 * samples >= below) launches nothing extra either.  The workspace does not grow.  Limits: v is biased low by about
 * sum(w^2) / sum(w)^2 (no Bessel correction), and a window that straddles a shadow edge on one surface reads it as noise. */
typedef struct pt_filter_spatial_opts {
  uint32_t below;      /* pixels with fewer samples than this take the estimate; 0 = off (default), PT_FILTER_SPATIAL_ALL = all */
  int32_t radius;      /* R: the window is (2R+1)^2, 1 .. 3 (default 2)                                                      */
  int32_t reserved[2]; /* must be 0                                                                                         */
} pt_filter_spatial_opts;
#define PT_FILTER_SPATIAL_ALL 0xFFFFFFFFu
#define PT_FILTER_SPATIAL_DEFAULT_RADIUS 2
void pt_filter_spatial_opts_default(pt_filter_spatial_opts* opts); /* below 0 (off), radius 2 */
/* The host checks of pt_filter_set_spatial alone (no device, no filter): PT_EINVAL naming the field for a null opts, a radius
 * outside 1 .. 3 (whatever `below` is) and a non-zero reserved word. */
int pt_filter_spatial_check(const pt_filter_spatial_opts* opts);
/* Switches the estimate of a filter on (below > 0) or off (below == 0, or opts == NULL).  Every value is checked before anything
 * else (pt_filter_spatial_check); a refused call leaves the filter as it was.  Touches no device.  It holds for every later
 * pt_filter_enqueue / _run / _enqueue_frames / _run_frames of the filter; a batch has no count image, so the uniform `samples`
 * decides for all its frames, and it stays the loop of single calls bit for bit. */
int pt_filter_set_spatial(pt_filter* f, const pt_filter_spatial_opts* opts);

/* ---- temporal accumulation: reproject and blend the frames of a fly-through ------------------ */
/* The temporal stage of SVGF in front of the filter above; no counterpart in the reference.  A session belongs to one frame
 * size and carries, from call to call, what the earlier frames accumulated: two history images used ping-pong, each three
 * float4 per pixel {colour, s2}, {normal, z}, {albedo, count} (96 bytes of workspace per pixel, pt_temporal_workspace_bytes), and
 * the previous call's camera.  A call works IN PLACE on a device frame [height][width][14] of uniform sample count n: it
 * rewrites channels 0-2 (colour) and 10 (the colour's per-sample variance) and leaves channels 3-9 and 11-13 untouched byte for
 * byte; the optional count image (uint32 [height][width]) receives every pixel's accumulated count and goes straight into
 * pt_filter_enqueue.  EXACT code: DENOISER.md, "Temporal accumulation", states the definition operation by operation and the
 * kernel equals its float32 restatement (tests/temporal_model.py) bit for bit.  Deterministic: two runs give the same bits.
 *   host      P = inverse of M = [B0 | B1-B0 | B2-B0] (columns, B0..B3 the corners of basis), by cofactors in double, rounded
 *             to float (pt_temporal_camera).  A primary direction is d = M (1, sy, v)^T, so P (X - eye) = t (1, sy, v)^T.
 *   pixel     (row r, column c) with depth z = ch9:  X = eye + d z for the unjittered d of the pixel (sy = c / height, v = 1 -
 *             r / width);  (alpha, beta, gamma) = P' (X - eye') with the PREVIOUS camera;  cc = (beta / alpha) height, rr = (1 -
 *             gamma / alpha) width;  the four bilinear taps around (rr, cc) of the history, a tap valid when it lies inside the
 *             frame, holds a count > 0 and |z' - alpha| <= depth_tol alpha, n' . n >= normal_tol, |alb' - alb|^2 <= albedo_tol;
 *             with Ws = the valid taps' weight >= min_weight the history is (hC, hs2, hN) = the taps' weighted means, hN capped
 *             at history_cap; otherwise, and where z <= 0 or alpha <= 0 or (rr, cc) is outside, the pixel restarts (hN = 0).
 *   blend     tot = hN + n;  colour = hC + (n / tot) (C - hC);  ch10 = the exact two-group merge of the sample variances:
 *             (hs2 max(hN - 1, 0) + ch10 (n - 1) + (lum(C) - lum(hC))^2 hN n / tot) / (tot - 1);  count = floor(tot + 0.5).
 * The first call of a session and the first after pt_temporal_reset pass the frame through (its own bits, count n).
 * Limits: silhouette pixels carry mixed depths and normals and mostly restart; sky pixels (z <= 0) never accumulate; the scene
 * must not change between calls except through the _scene calls below, or without a reset.  One session's calls share its workspace and are ordered by the stream: do
 * not run two of them concurrently on different streams. */
typedef struct pt_temporal_opts {
  float history_cap;  /* the accumulated count never exceeds this many samples, >= 1 (default 256)            */
  float depth_tol;    /* relative depth stop, finite and > 0 (default 0.02)                                   */
  float normal_tol;   /* smallest n' . n of a valid tap, -1 .. 1 (default 0.9)                                */
  float albedo_tol;   /* largest squared albedo distance of a valid tap, finite and > 0 (default 0.01)        */
  float min_weight;   /* smallest bilinear weight of the valid taps that keeps the history, (0, 1] (default 0.25) */
  int32_t reserved;   /* must be 0                                                                            */
} pt_temporal_opts;
typedef struct pt_temporal pt_temporal; /* opaque: the options, the history and the previous camera of one frame size */
void pt_temporal_opts_default(pt_temporal_opts* opts);
/* opts may be NULL (= defaults).  Every option and size is validated BEFORE a device is touched (the size limits are
 * pt_filter_create's); a bad value is PT_EINVAL naming the argument.  Allocates the workspace on the current device. */
int pt_temporal_create(int width, int height, const pt_temporal_opts* opts, pt_temporal** out);
int pt_temporal_destroy(pt_temporal* t);
/* Forgets the history: the next frame passes through.  Call it when the scene changes. */
int pt_temporal_reset(pt_temporal* t);
int pt_temporal_workspace_bytes(const pt_temporal* t, uint64_t* bytes);
/* The host step alone (no device): P_out = the row-major inverse above.  PT_EINVAL for a determinant that is zero or not
 * finite, and for a basis whose B1 + B2 - B0 - B3 exceeds 1e-3 |B0| in any component (the mapping assumes the parallelogram
 * that pt_camera_basis produces). */
int pt_temporal_camera(const float basis[12], float P_out[9]);
/* Accumulates the device frame d_frame of `samples` >= 1 samples per pixel, rendered with (basis, eye), asynchronous on
 * hip_stream (NULL = default stream).  d_counts may be NULL.  A null accumulator, frame, basis or eye, samples < 1, a basis
 * pt_temporal_camera refuses or a non-finite eye is PT_EINVAL naming the argument; nothing is launched and the session keeps
 * its state. */
int pt_temporal_enqueue(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                        void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around it. */
int pt_temporal_run(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], uint32_t* d_counts,
                    float* ms_out);
/* n frames in order, bit for bit what
 *   for k in 0 .. n-1: pt_temporal_enqueue(t, d_frames + k * frame_stride, samples, bases + 12 k, eyes + 3 k, NULL, s)
 * does (frame k reads what frame k-1 wrote, so it is n launches); d_counts receives the counts of the LAST frame.  Strides are in
 * floats and may leave gaps (frame_stride >= width x height x 14), so the output of pt_renderer_enqueue_frames passes straight
 * in.  n_frames < 1, a stride too small, and everything pt_temporal_enqueue refuses, for any frame, is PT_EINVAL and nothing is
 * launched. */
int pt_temporal_enqueue_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                               const float* eyes, int samples, uint32_t* d_counts, void* hip_stream);
int pt_temporal_run_frames(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                           const float* eyes, int samples, uint32_t* d_counts, float* ms_out);

/* -- moving spheres: a motion vector per pixel (DENOISER.md, "Moving spheres") --
 * A motion image is a device image [height][width] of four floats {mx, my, mz, w}: the sphere that the CENTRE ray of the pixel
 * hits first in this frame's scene has index w and has moved by m since the previous frame; a miss is {0, 0, 0, -1}.  With a
 * motion image the pixel step above carries the world point back before the previous camera looks at it: X = eye + d z, then
 * Xp = X - m, and (alpha, beta, gamma) = P' (Xp - eye'); taps, stops and blend are unchanged.  The depth stop needs no change:
 * alpha is the distance parameter, in the previous camera, of the point where the surface was, which is what the history holds
 * there if the same sphere was visible.  A zero motion image gives the bits of the static call; a pixel whose centre ray misses is
 * treated as static; background uncovered by a departing sphere reprojects onto history that holds the sphere, fails the stops and
 * restarts; a NaN or infinite motion component restarts the pixel as a NaN depth does.  EXACT code, restated in
 * tests/temporal_motion_model.py.
 *   motion    d = the unjittered primary direction of the pixel, NOT normalised; the nearest hit of (eye, d) among the n spheres
 *             of h_now by the reference's intersectSphere / intersectScene (src/pathtrace.cu:72-107): double where its literals
 *             force double, float elsewhere, t > 0 && t < tNearest from 1000000.0f, strict <, so the lowest index wins a tie;
 *             on a hit of sphere i: m = h_now[i].pos - h_prev[i].pos (one float subtraction per component), w = (float)i.
 * The kernel tests every sphere for every pixel (no grid), PT_MOTION_CHUNK spheres per round through LDS.
 * Limits: rigid translation only (a changed radius is refused); the centre ray decides a pixel's sphere, so silhouettes restart
 * as they do anyway; a moving sphere's shadow and its indirect light on static surfaces are not followed and lag by up to
 * history_cap samples: use a small cap for animated scenes, or the responsive history below. */
#define PT_MOTION_CHUNK 256
/* The host checks of pt_temporal_motion alone (no device, no session): PT_EINVAL naming the argument for a null pointer, n
 * outside 1 .. 65535, a field of either array that is not finite (colour and emission are checked, though not read), a radius
 * that is not bitwise equal in both arrays ("reset the session"), a non-finite eye and a basis pt_temporal_camera refuses. */
int pt_temporal_scene_check(const pt_sphere* h_now, const pt_sphere* h_prev, int n, const float basis[12], const float eye[3]);
/* The motion image of the HOST arrays h_now, h_prev (n spheres each, index-matched) under the camera (basis, eye) into d_motion
 * (width x height x 4 floats), asynchronous on hip_stream.  A null accumulator or d_motion and everything
 * pt_temporal_scene_check refuses is PT_EINVAL, checked before a device is touched; nothing is launched.  The spheres travel
 * through a pinned staging buffer of the session (32 bytes per sphere on the device, 128 pinned; not part of
 * pt_temporal_workspace_bytes), so the arrays may be reused as soon as the call returns and no call waits for the device
 * unless four earlier uploads of the session are still pending (the call then waits for the oldest one's event).  The staging
 * is allocated by the first call that needs it and again, at twice the size, by a call with more spheres than it holds: such
 * a call allocates (hipMalloc, hipHostMalloc; do not make it under stream capture) but does not wait for the device's work --
 * the outgrown buffers, which enqueued work may still read, are kept until pt_temporal_destroy.  Call once with the largest
 * scene up front to have no allocation later.  Neither the history nor the remembered scene is touched. */
int pt_temporal_motion(pt_temporal* t, const pt_sphere* h_now, const pt_sphere* h_prev, int n, const float basis[12], const float eye[3],
                       float* d_motion, void* hip_stream);
/* pt_temporal_enqueue / pt_temporal_run with a motion image; d_motion == NULL is exactly pt_temporal_enqueue / pt_temporal_run
 * (the same kernel, the same bits). */
int pt_temporal_enqueue_motion(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const float* d_motion,
                               uint32_t* d_counts, void* hip_stream);
int pt_temporal_run_motion(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const float* d_motion,
                           uint32_t* d_counts, float* ms_out);
/* The form for animated scenes: accumulates d_frame, rendered from the n HOST spheres h_spheres.  The session keeps a host copy
 * of the scene of its previous call, builds the motion image (this scene against that one) into a buffer of its own -- 16 bytes
 * per pixel, allocated by the first call that needs it and reported by pt_temporal_workspace_bytes from then on -- and
 * accumulates with it: two launches.  The first call of a session and the first after pt_temporal_reset pass the frame through
 * and only remember the scene.  Everything pt_temporal_enqueue refuses, a null h_spheres, n outside 1 .. 65535, a field that is
 * not finite, an n that differs from the remembered scene's and a radius that differs from it ("reset the session") are
 * PT_EINVAL; nothing is launched and the session, its remembered scene included, is as it was.  The calls above without a scene
 * may be mixed in: they forget the remembered scene, so the next _scene call accumulates with zero motion (the static kernel)
 * and remembers its scene.  A session that never uses the calls of this section allocates nothing for them. */
int pt_temporal_enqueue_scene(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const pt_sphere* h_spheres,
                              int n, uint32_t* d_counts, void* hip_stream);
int pt_temporal_run_scene(pt_temporal* t, float* d_frame, int samples, const float basis[12], const float eye[3], const pt_sphere* h_spheres,
                          int n, uint32_t* d_counts, float* ms_out);
/* n_frames frames with their scenes h_scenes [n_frames][n], bit for bit the loop of pt_temporal_enqueue_scene calls (two
 * launches per frame, one for a frame that passes through or has no remembered scene); d_counts receives the counts of the LAST
 * frame.  Every frame and scene is checked before the first launch. */
int pt_temporal_enqueue_frames_scenes(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                                      const float* eyes, const pt_sphere* h_scenes, int n, int samples, uint32_t* d_counts, void* hip_stream);
int pt_temporal_run_frames_scenes(pt_temporal* t, int n_frames, float* d_frames, size_t frame_stride_floats, const float* bases,
                                  const float* eyes, const pt_sphere* h_scenes, int n, int samples, uint32_t* d_counts, float* ms_out);

/* -- responsive history: a fast history that clamps the long one (DENOISER.md, "Responsive history") --
 * What a moving sphere does to OTHER surfaces -- its shadow, its indirect light -- is not followed by the motion image and would
 * lag by up to history_cap samples.  With anti-lag on, the session keeps a second history of at most fast_cap samples beside the
 * long one (two more images used ping-pong, one float4 {colour, count} per pixel each: 32 more bytes of workspace per pixel), and
 * after every accumulate launch a second launch clamps the long history's colour, per pixel and channel, into mu +- clamp_sigma x
 * sigma of the fast colours in the (2 clamp_radius + 1)^2 window around the pixel.  Stable light lies inside that box and keeps
 * all its samples; changed light is pulled to the recent frames.  EXACT code, restated in tests/temporal_antilag_model.py:
 *   fast      the same four taps, validity and weights as the pixel step above; {fC', fn'} = the tap's fast float4, selected to 0
 *             when invalid; fhC = sum(w fC') / Ws, fhN = min(sum(w fn') / Ws, fast_cap) when Ws >= min_weight, else 0;
 *             ftot = fhN + n;  fC = fhC + (n / ftot) (C - fhC);  {fC, ftot} goes into the other fast image.
 *   rectify   not issued on a call without history.  Window rows r-R .. r+R, columns c-R .. c+R in row-major order, only the m
 *             taps inside the frame; per channel S1 = sum x, S2 = sum (x x) sequentially from +0; mu = S1 / m; v = S2 / m - mu mu;
 *             var = v > 0 ? v : 0; sigma = sqrt(var); lo = mu - k sigma; hi = mu + k sigma.  A pixel is active iff tot > ftot;
 *             an active pixel's colour x becomes x < lo ? lo : (x > hi ? hi : x) in channels 0-2 of the frame and in the long
 *             history; channel 10, the counts and the fast image are not touched, an inactive pixel is not written.
 * Limits: the window ignores surfaces (a silhouette widens sigma, so the clamp only acts less there); a clamped pixel keeps its
 * count and its variance; a +-Inf in a window drags its neighbours' bounds to it (a NaN switches their clamp off). */
typedef struct pt_temporal_antilag_opts {
  float fast_cap;       /* 0 = off (the session of the sections above).  Otherwise >= 1 and < the session's history_cap */
  float clamp_sigma;    /* k: half-width of the clamp box in standard deviations, finite, > 0 (default 1)             */
  int32_t clamp_radius; /* R: the window is (2R+1)^2, 1 .. 3 (default 1)                                              */
  int32_t reserved;     /* must be 0                                                                                  */
} pt_temporal_antilag_opts;
#define PT_ANTILAG_DEFAULT_SIGMA 1.0f
#define PT_ANTILAG_DEFAULT_RADIUS 1
void pt_temporal_antilag_opts_default(pt_temporal_antilag_opts* opts); /* fast_cap 0 (off), clamp_sigma and clamp_radius as above */
/* The host checks of pt_temporal_set_antilag alone (no device, no session) for a session of the given history_cap: PT_EINVAL
 * naming the field for a null opts, fast_cap that is neither 0 nor in [1, history_cap), clamp_sigma that is not finite and > 0,
 * clamp_radius outside 1 .. 3 and reserved != 0. */
int pt_temporal_antilag_check(const pt_temporal_antilag_opts* opts, float history_cap);
/* Switches the responsive history of a session on (fast_cap > 0) or off (fast_cap == 0: today's launches; the fast images may
 * stay allocated and reported).  Accepted only while the session holds no history -- before its first frame or right after
 * pt_temporal_reset -- otherwise PT_EINVAL "reset the session".  Every value is checked before a device is touched
 * (pt_temporal_antilag_check); a refused call leaves the session as it was.  Switching on allocates the fast images (hipMalloc:
 * not under stream capture), reported by pt_temporal_workspace_bytes from then on.  Every enqueue / run call of the session,
 * with or without a motion image or a scene, then takes the FAST form; a batch stays the loop of single calls bit for bit. */
int pt_temporal_set_antilag(pt_temporal* t, const pt_temporal_antilag_opts* opts);
/* Debug view: copies the fast image the last call wrote, [height][width][4] floats {fast rgb, fast count}, into d_out,
 * asynchronous on hip_stream.  PT_EINVAL if anti-lag is off or no frame has run since the session was made or reset. */
int pt_temporal_fast(pt_temporal* t, float* d_out, void* hip_stream);

/* ---- tone mapping: metered exposure, a filmic curve and sRGB bytes ---------------------------- */
/* The stage between a frame of linear radiance and a picture; no counterpart in the reference, whose display path is the clamp
 * of pt_display_pack.  A session belongs to one frame size and keeps ONE float on the device, the exposure e, so no call
 * synchronises with the host.  EXACT code: every operation below is a float32 add, multiply, divide or compare (no
 * contraction), an integer sum or a table lookup, and the kernels equal the float32 restatement (tests/tonemap_model.py) bit
 * for bit; the reductions are sums of integers, so their order cannot change a bit.  DENOISER.md, "Tone mapping", says the same.
 *   input     device floats [height][width][pixel_stride], pixel_stride in 3 .. 64, colour c in the first three floats of a
 *             pixel: stride 14 is a frame, stride 3 the d_rgb of pt_filter_* / pt_denoiser_*.  The input is never written.
 *   output    device uint32 [height][width], r | g << 8 | b << 16 | 255 << 24.
 *   lum(c)    (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z, left to right in float32.
 *   1 meter   (only with exposure = 0, "auto")  a pixel is metered when the bit pattern of L = lum(c) lies in [bits(2^-20),
 *             0x7F7FFFFF], that is L is finite and >= 2^-20: NaN, inf, zero, negative and black sky pixels do not count.
 *             S = the sum of the metered pixels' bit patterns as uint64, K = their number;  m = S / K as an integer division;
 *             Lavg = the float whose bits are (uint32)m;  target = key / Lavg, a float32 divide.  With K = 0 target is the
 *             previous exposure, or 1 with no history.  (Averaging bit patterns averages a piecewise-linear log2, so Lavg is
 *             a geometric mean: log2 Lavg lies within 0.0861 of the true mean log2, +-6 % in exposure, for a sum that is exact
 *             in any order.  2^26 pixels x 2^31 stays below 2^64.)
 *   2 adapt   first frame, first after pt_tonemap_reset, or adapt = 1:  e = target, the same bits;  otherwise d = target - e;
 *             e = e + adapt d, two float32 roundings.  With a fixed exposure e is the option and neither meter nor adapt runs.
 *   3 map     per channel  x = c e;  x = x > 0 ? x : 0 (NaN becomes 0);  x = x < 65504 ? x : 65504;
 *             PT_TONEMAP_CLAMP     y = x
 *             PT_TONEMAP_REINHARD  Lx = lum(x);  s = (1 + Lx / (white white)) / (1 + Lx);  y = x s   (on luminance: hue is kept)
 *             PT_TONEMAP_ACES      y = (x (2.51f x + 0.03f)) / (x (2.43f x + 0.59f) + 0.14f)         (Narkowicz's rational fit)
 *             then y = y < 1 ? y : 1 (NaN becomes 1).
 *   4 encode  PT_ENCODE_SRGB    code = the number of k in 1 .. 255 with T[k] <= y, where T[k] is the float32 nearest to
 *                               u <= 0.04045 ? u / 12.92 : pow((u + 0.055) / 1.055, 2.4) formed in double at u = (k - 0.5) / 255:
 *                               the correctly rounded 8-bit sRGB code.  The table is built once on the host, kept in LDS and
 *                               searched in eight steps; there is no powf on the device.
 *             PT_ENCODE_LINEAR  (unsigned char)((double)y * 255.0), the display packer's own line.
 * With PT_TONEMAP_CLAMP, exposure 1 and PT_ENCODE_LINEAR the three colour bytes are exactly those of pt_display_pack.  There is
 * no dithering.  Launches: a fixed exposure is ONE launch per call; auto is three (meter: per-workgroup partial (S, K) into the
 * workspace; adapt: one workgroup adds them and carries e; map).  No float atomics, no memset, no host synchronisation.
 * Workspace: 1040 bytes (table, state) + per frame of a group 16 bytes per 256 pixels + 4 (pt_tonemap_workspace_bytes).  One
 * session's calls share its workspace and state and are ordered by the stream: do not run two of them concurrently. */
#define PT_TONEMAP_CLAMP 0
#define PT_TONEMAP_REINHARD 1
#define PT_TONEMAP_ACES 2
#define PT_ENCODE_SRGB 0
#define PT_ENCODE_LINEAR 1
typedef struct pt_tonemap_opts {
  int32_t curve;       /* PT_TONEMAP_CLAMP, _REINHARD or _ACES (default ACES)                                    */
  int32_t encode;      /* PT_ENCODE_SRGB (default) or PT_ENCODE_LINEAR                                           */
  float exposure;      /* 0 = auto (default): metered and adapted on the device; else finite and > 0: fixed      */
  float key;           /* auto: the luminance the geometric mean is mapped to, finite and > 0 (default 0.18)     */
  float white;         /* Reinhard: the luminance that maps to 1, 1e-18 .. 1e18 (default 4)                      */
  float adapt;         /* auto: share of the way to the target taken per frame, (0, 1] (default 1 = at once)     */
  int32_t max_frames;  /* frames per group, >= 1 (default 1)                                                     */
  int32_t reserved[2]; /* must be 0                                                                              */
} pt_tonemap_opts;
typedef struct pt_tonemap pt_tonemap; /* opaque: the options, the table, the exposure and the partials of one frame size */
void pt_tonemap_opts_default(pt_tonemap_opts* opts);
/* opts may be NULL (= defaults).  Every option and size is validated BEFORE a device is touched (the size limits are
 * pt_filter_create's, max_frames' those of pt_filter_reserve_frames); a bad value is PT_EINVAL naming the argument.  Allocates
 * the workspace on the current device. */
int pt_tonemap_create(int width, int height, const pt_tonemap_opts* opts, pt_tonemap** out);
int pt_tonemap_destroy(pt_tonemap* t);
/* Forgets the exposure: the next frame's exposure is its own target. */
int pt_tonemap_reset(pt_tonemap* t);
int pt_tonemap_workspace_bytes(const pt_tonemap* t, uint64_t* bytes);
/* Grows the workspace for groups of up to max_frames frames, with pt_filter_reserve_frames' limits and rules; the exposure is kept. */
int pt_tonemap_reserve_frames(pt_tonemap* t, int max_frames);
/* Host only: out[k - 1] = T[k] of the encode step, k = 1 .. 255. */
int pt_tonemap_srgb_table(float out[255]);
/* Maps the device image d_src to d_rgba8, asynchronous on hip_stream (NULL = default stream).  A null session, source or
 * destination, or a pixel_stride outside 3 .. 64, is PT_EINVAL naming the argument; nothing is launched and the session keeps
 * its state. */
int pt_tonemap_enqueue(pt_tonemap* t, const float* d_src, int pixel_stride, uint32_t* d_rgba8, void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around it. */
int pt_tonemap_run(pt_tonemap* t, const float* d_src, int pixel_stride, uint32_t* d_rgba8, float* ms_out);
/* n frames in order, bit for bit what
 *   for k in 0 .. n-1: pt_tonemap_enqueue(t, d_src + k * src_stride_floats, pixel_stride, d_rgba8 + k * dst_stride_pixels, s)
 * does, the adaptation carried from frame to frame included.  A group of up to max_frames frames goes out in three launches
 * (one with a fixed exposure): meter all its frames, one workgroup adapts them in order, map all its frames.  Strides may leave
 * gaps (src_stride_floats >= width x height x pixel_stride, dst_stride_pixels >= width x height).  n_frames < 1, a stride too
 * small, and everything pt_tonemap_enqueue refuses is PT_EINVAL and nothing is launched. */
int pt_tonemap_enqueue_frames(pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride,
                              uint32_t* d_rgba8, size_t dst_stride_pixels, void* hip_stream);
int pt_tonemap_run_frames(pt_tonemap* t, int n_frames, const float* d_src, size_t src_stride_floats, int pixel_stride,
                          uint32_t* d_rgba8, size_t dst_stride_pixels, float* ms_out);
/* Synchronous (it waits for the device): *out = the e of the last frame; the option with a fixed exposure; 1 before the first
 * frame and after a reset. */
int pt_tonemap_exposure(pt_tonemap* t, float* out);

/* ---- frame comparison: clamped MSE, relMSE and SSIM against a reference ------------------------ */
/* How far an image is from its reference, measured on the device: the stage beside the four above, for whoever chooses a filter
 * sigma, a denoiser precision, an adaptive tolerance or a temporal cap.  The reference renders every pose twice (2 spp and
 * 20000 spp) and judges one against the other off the device; this stage keeps both frames where they are.  A session belongs
 * to one frame size.  It reads two device images and writes neither; the results stay on the device until pt_compare_result
 * asks for them.  EXACT code, like the tone mapper's: float32 adds, multiplies, divides and compares without contraction, and
 * integer sums, so the kernels equal the float32 restatement (tests/compare_model.py) bit for bit and the sums do not depend
 * on their order.  DENOISER.md, "Frame comparison", says the same.
 *   input     two device images [height][width][pixel_stride], each with its own pixel_stride in 3 .. 64, colour in the first
 *             three floats of a pixel (14: a frame, 3: an rgb image).
 *   1 sanitise  per channel x = c > 0 ? c : 0 (NaN becomes 0);  x = x < 65504 ? x : 65504: a for the image, b for the reference.
 *             A pixel with a non-finite colour channel in either input counts once in `nonfinite`.  Display values:
 *             a' = a < 1 ? a : 1, b' likewise.
 *   2 MSE     per channel d = a' - b';  t = d d;  per pixel m = (t0 + t1) + t2 <= 3: what a display shows.
 *   3 relMSE  per channel d = a - b;  t = (d d) / (b b + 0.01f);  t = t < 1024 ? t : 1024, and a channel that hit the cap counts
 *             in `saturated`;  per pixel r = (t0 + t1) + t2 <= 3072.
 *   4 SSIM    Wang et al.: 11 x 11 Gaussian window, sigma 1.5, L = 1, C1 = 0.01f 0.01f, C2 = 0.03f 0.03f, on la = lum(a') and
 *             lb = lum(b') (lum: the tone mapper's).  The 11 weights w are formed on the host in double, exp(-(k - 5)^2 / 4.5)
 *             divided by their sum, and rounded to float32 (pt_compare_ssim_weights).  The filter is separable, first along a
 *             row, then along a column, on the five quantities la, lb, la la, lb lb, la lb;  a pass is
 *             v = w[0] q[-5];  v = v + w[k] q[k - 5] for k = 1 .. 10, and coordinates clamp to the frame (edges replicate), so
 *             every pixel has a window and a 1 x 1 frame is legal.  With the filtered values ua, ub, Eaa, Ebb, Eab:
 *             va = Eaa - ua ua;  vb = Ebb - ub ub;  cab = Eab - ua ub;
 *             s = ((2 (ua ub) + C1) (2 cab + C2)) / (((ua ua + ub ub) + C1) ((va + vb) + C2)).
 *   5 sums    per pixel qm = (uint64)floor((double)m 2^34), qr = (uint64)floor((double)r 2^24), qs = (int64)floor((double)s 2^32);
 *             a frame's three sums are 64-bit integers (each term is below 2^36 in size, a group has at most 2^26 pixels).
 *   6 result  mse = (double)sum qm / 2^34 / (3 pixels);  rms = sqrt(mse);  psnr = mse > 0 ? -10 log10(mse) : +inf;
 *             relmse = (double)sum qr / 2^24 / (3 pixels);  ssim = (double)sum qs / 2^32 / pixels.
 *   7 map     optional: d_map[3 p ..] = (m, r, s) of pixel p, an error picture.
 * Launches: two per group of up to max_frames frames (one workgroup per 16 x 16 tile writes its partial sums into the
 * workspace; one workgroup adds them into the frames' records).  No float atomics, no memset, no host synchronisation.
 * Workspace: per frame of a group 32 bytes per tile, and 40 bytes per frame of the largest call so far
 * (pt_compare_workspace_bytes).  One session's calls share its workspace and are ordered by the stream: do not run two of them
 * concurrently. */
typedef struct pt_compare_opts {
  int32_t max_frames;  /* frames per group, >= 1 (default 1) */
  int32_t reserved[3]; /* must be 0                          */
} pt_compare_opts;
typedef struct pt_compare_values {
  uint64_t sum_mse;    /* the sum of qm                                        */
  uint64_t sum_relmse; /* the sum of qr                                        */
  int64_t sum_ssim;    /* the sum of qs                                        */
  uint64_t pixels;     /* width x height                                       */
  uint64_t saturated;  /* channels whose relMSE term hit the cap of 1024       */
  uint64_t nonfinite;  /* pixels with a NaN or an infinity in either input     */
  double mse, rms, psnr, relmse, ssim; /* step 6                               */
} pt_compare_values;
typedef struct pt_compare pt_compare; /* opaque: the weights, the partial sums and the records of one frame size */
void pt_compare_opts_default(pt_compare_opts* opts);
/* opts may be NULL (= defaults).  Every option and size is validated BEFORE a device is touched (the size limits are
 * pt_filter_create's, max_frames' those of pt_filter_reserve_frames); a bad value is PT_EINVAL naming the argument.  Allocates
 * the workspace on the current device. */
int pt_compare_create(int width, int height, const pt_compare_opts* opts, pt_compare** out);
int pt_compare_destroy(pt_compare* c);
int pt_compare_workspace_bytes(const pt_compare* c, uint64_t* bytes);
/* Grows the workspace for groups of up to max_frames frames, with pt_filter_reserve_frames' limits and rules; the results of
 * the last call are kept. */
int pt_compare_reserve_frames(pt_compare* c, int max_frames);
/* Host only: the eleven float32 weights of step 4. */
int pt_compare_ssim_weights(float out[11]);
/* Compares the device image d_img with its reference d_ref, asynchronous on hip_stream (NULL = default stream).  d_map may be
 * NULL; otherwise it receives width x height x 3 floats.  A null session, image or reference, or a pixel stride outside
 * 3 .. 64, is PT_EINVAL naming the argument; nothing is launched and the results of the last call stay as they were. */
int pt_compare_enqueue(pt_compare* c, const float* d_img, int img_pixel_stride, const float* d_ref, int ref_pixel_stride, float* d_map,
                       void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around it. */
int pt_compare_run(pt_compare* c, const float* d_img, int img_pixel_stride, const float* d_ref, int ref_pixel_stride, float* d_map,
                   float* ms_out);
/* n frames, bit for bit what n single calls give: frame k compares d_img + k * img_stride_floats with
 * d_ref + k * ref_stride_floats and writes its map to d_map + k * map_stride_floats.  ref_stride_floats == 0 is ONE reference
 * for all n frames: the convergence curve of a session's passes, or of a fly-through's frames, against one converged picture.
 * Otherwise strides may leave gaps (img_stride_floats >= width x height x img_pixel_stride, likewise the reference's;
 * map_stride_floats >= width x height x 3 when d_map is given).  A group of up to max_frames frames goes out in two launches.
 * A call with more frames than any call before first makes room for their records, which waits for the device once.
 * n_frames < 1, a stride too small, and everything pt_compare_enqueue refuses is PT_EINVAL and nothing is launched. */
int pt_compare_enqueue_frames(pt_compare* c, int n_frames, const float* d_img, size_t img_stride_floats, int img_pixel_stride,
                              const float* d_ref, size_t ref_stride_floats, int ref_pixel_stride, float* d_map, size_t map_stride_floats,
                              void* hip_stream);
int pt_compare_run_frames(pt_compare* c, int n_frames, const float* d_img, size_t img_stride_floats, int img_pixel_stride, const float* d_ref,
                          size_t ref_stride_floats, int ref_pixel_stride, float* d_map, size_t map_stride_floats, float* ms_out);
/* Synchronous (it waits for the device): *out = steps 5 and 6 for frame frame_index of the last accepted call (0 for a single
 * call).  A frame_index outside the last call's frames, also before the first call, is PT_EINVAL. */
int pt_compare_result(pt_compare* c, int frame_index, pt_compare_values* out);

/* ---- training patches: pre-process, score and gather on the device ------------------------------ */
/* From a (train frame, target image) pair on the device, what a CNN's data loader consumes: the pre-processed inputs
 * [N][14][P][P] and the clamped targets [N][3][P][P] of N square patches, and the score by which patches are chosen.  This is
 * what the reference's denoise_cnn/load_data.py computes off the device in float64 (load_exr_data's pre-processing, get_score,
 * the crops of get_patches); the pre-processing here is the one pt_denoiser_* applies at inference, bit for bit
 * (tests/denoise_restatement.py: preprocess).  Training itself stays with the caller.  EXACT code, like the tone mapper's and
 * the comparison's: float32 divides and compares without contraction and integer sums, so the kernels equal the float32
 * restatement (tests/patches_model.py) bit for bit and the sums do not depend on their order.  DENOISER.md, "Training patches",
 * says the same.
 *   input     a train frame [height][width][14] (pixel stride 14 only) and a target image [height][width][gt_pixel_stride],
 *             stride 3 .. 64, colour in the first three floats.  Neither is ever written.
 *   session   belongs to (width, height, patch P, max_patches K): 1 <= P <= min(width, height, 1024), 1 <= K <= 65535,
 *             K P P <= 2^26.
 *   indices   "row" and "column" are the frame's first and second index as it lies in memory: the orientation in which the
 *             project's own Denoiser sees a frame.  The reference's tensors are the transpose (swapaxes(0, 2)), in training
 *             and in inference alike: the one deliberate difference.
 *   1 divisors  m_k = the maximum of channel k in 9 .. 13 over the WHOLE train frame, by fmaxf from -inf (NaNs are ignored);
 *             div_k = (float)(0.00316 + (double)m_k);  EPS = 0.00316f.
 *   2 pixel   x[0..2] = colour / (EPS + albedo), an IEEE float32 divide;  x[3..8] unchanged;  x[9..13] = c / div_k.
 *   3 score   of the patch with corner (cx, cy), 0 <= cx <= width - P, 0 <= cy <= height - P.  Two populations of 3 P P values:
 *             the pre-processed colour x[0..2] and the normal x[3..5].  Per value: colour v = x > 0 ? x : 0 (NaN becomes 0),
 *             v = v < 65504 ? v : 65504;  normal NaN becomes 0, then clamped to +-65504;  q = (int64)floor((double)v 2^20).
 *             Per population, with a = |q|, ah = a >> 18, al = a & (2^18 - 1):  S1 = sum q (int64);  A = sum ah ah,
 *             B = sum ah al, C = sum al al (uint64): all exact in 64 bits for P <= 1024.  pt_patches_result then forms, in
 *             128-bit integers, S2 = A 2^36 + B 2^19 + C (= sum q q), N = 3 P P, num = N S2 - S1 S1, and
 *             var = ((double)num / (double)(N N)) / 2^40 (the conversion rounds to nearest even, N N is exact);
 *             score = var_colour + var_normal.  This is get_score's np.var(colour) + np.var(normal), a pooled variance per
 *             group of three channels, made independent of the order of summation and bounded: where the reference's float64
 *             value would be inf or NaN this score is finite.
 *   4 gather  inputs[k][c][j][i] = x[c] of pixel (cy_k + j, cx_k + i): the unsanitised value of step 2, NaNs pass as inference
 *             would see them.  targets[k][c][j][i] = t, t = g > 0 ? g : 0;  t = t < 1 ? t : 1, g the target's colour:
 *             np.clip(g, 0, 1) except that NaN becomes 0.  Both float32 and contiguous.
 * Corners are a HOST array of n (x, y) int32 pairs.  Every corner is validated on the host before anything is launched: a
 * corner outside 0 .. width - P / 0 .. height - P, n < 1 or n > max_patches is PT_EINVAL naming the index and the value, so no
 * kernel is handed an address outside the caller's images.  They reach the device through a pinned buffer of the session and an
 * asynchronous copy on the call's stream; the caller's array may be reused when the call returns.
 * Launches: prepare one (per-workgroup maxima; whoever divides folds them), score two (per patch, one workgroup per 1024 pixels
 * writes its eight sums; one workgroup per patch adds them into the patch's record), gather one.  No atomics, no memset, no
 * host synchronisation.  One session's calls share its workspace and are ordered by the stream: do not run two concurrently. */
typedef struct pt_patches_opts {
  int32_t patch;       /* P, the side of a patch in pixels (default 64) */
  int32_t max_patches; /* K, the most patches of one call (default 64)  */
  int32_t reserved[2]; /* must be 0                                     */
} pt_patches_opts;
typedef struct pt_patches_values {
  int64_t colour_s1;  /* S1 of the pre-processed colour */
  uint64_t colour_a, colour_b, colour_c; /* A, B, C     */
  int64_t normal_s1;  /* S1 of the normal               */
  uint64_t normal_a, normal_b, normal_c;
  uint64_t values;    /* N = 3 P P                      */
  double var_colour, var_normal, score; /* step 3       */
} pt_patches_values;
typedef struct pt_patches pt_patches; /* opaque: the maxima, the corners, the partial sums and the records */
void pt_patches_opts_default(pt_patches_opts* opts);
/* opts may be NULL (= defaults).  Every option and size is validated BEFORE a device is touched (the frame's size limits are
 * pt_filter_create's); a bad value is PT_EINVAL naming the argument.  Allocates the workspace on the current device. */
int pt_patches_create(int width, int height, const pt_patches_opts* opts, pt_patches** out);
int pt_patches_destroy(pt_patches* s);
int pt_patches_workspace_bytes(const pt_patches* s, uint64_t* bytes);
/* Step 1 for the frame d_train, asynchronous on hip_stream (NULL = default stream).  The maxima stay on the device.  A score or
 * a gather before the first prepare is PT_EINVAL.  A new frame needs a new prepare: score and gather take the same frame again,
 * and its CONTENT cannot be checked (the rule a progressive session has for its scene). */
int pt_patches_prepare(pt_patches* s, const float* d_train, void* hip_stream);
/* Step 3 for n corners, asynchronous; the records stay on the device until pt_patches_result asks for them.  A batch of n
 * patches gives the records of n single calls. */
int pt_patches_score(pt_patches* s, const float* d_train, int n, const int32_t* corners, void* hip_stream);
/* Synchronous (it waits for the device): *out = step 3 for patch patch_index of the last accepted score call.  A patch_index
 * outside that call's patches, also before the first call, is PT_EINVAL.  A gather in between changes nothing. */
int pt_patches_result(pt_patches* s, int patch_index, pt_patches_values* out);
/* Steps 2 and 4 for n corners, asynchronous: d_inputs receives n x 14 x P x P floats, d_targets (may be NULL; then d_gt and
 * gt_pixel_stride are not looked at) n x 3 x P x P.  A null session, frame or d_inputs, a null d_gt or a gt_pixel_stride
 * outside 3 .. 64 with d_targets given, is PT_EINVAL naming the argument; nothing is launched. */
int pt_patches_gather(pt_patches* s, const float* d_train, const float* d_gt, int gt_pixel_stride, int n, const int32_t* corners,
                      float* d_inputs, float* d_targets, void* hip_stream);
/* The same three, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events. */
int pt_patches_run_prepare(pt_patches* s, const float* d_train, float* ms_out);
int pt_patches_run_score(pt_patches* s, const float* d_train, int n, const int32_t* corners, float* ms_out);
int pt_patches_run_gather(pt_patches* s, const float* d_train, const float* d_gt, int gt_pixel_stride, int n, const int32_t* corners,
                          float* d_inputs, float* d_targets, float* ms_out);

/* ---- progressive rendering ------------------------------------------------------------ */
/* A still frame refined pass by pass.  The reference renders the same frame again and again while the camera rests
 * (src/main.cu:146-177: Render() of `spp` fresh samples, pathtrace.cu:212-256); a session instead ADDS samples to one frame.
 * A session belongs to one renderer and holds one still frame: one camera (basis + eye) and one scene.
 *  - pt_progressive_enqueue(p, spp, ...) adds spp >= 1 samples per pixel and writes the frame of ALL samples so far into d_out,
 *    in the renderer's layout and tile.  After a pass that leaves the session at n >= 2 samples, d_out is bit for bit the frame
 *    the first Render() of a fresh renderer with the same options produces at n spp, however n was split into passes.
 *  - Jitter: the reference jitters only when spp != 1 (pathtrace.cu:219-225).  A session cannot know its final count, so a
 *    session ALWAYS jitters.  Hence the one exception: the frame after a first pass of exactly one sample is the first sample
 *    of the jittered stream, not the reference's unjittered 1-spp frame.
 *  - Generator: a session starts from the seed, not from the renderer's persisted state (XORWOW xorwow_init(id + seed),
 *    philox key (seed, frame 0)).  Passes never touch the renderer's generator state or frame counter, and Render() calls
 *    between passes do not disturb the session.  pt_progressive_reset returns it to 0 samples.
 *  - d_out is output only: the state lives in the session's own record (PT_CHUNK_WORDS = 26 words per tile pixel, 104 B).
 *    The caller may denoise the frame in place, overwrite it, or pass a different buffer on every pass.
 *  - A pass whose camera (15 floats, compared bitwise), d_spheres or n_spheres differs from the session's first pass returns
 *    PT_EINVAL ("reset the session").  The CONTENT of the scene cannot be checked: it must not change during a session.  A
 *    total above INT_MAX samples (the reference's counts are int) and spp < 1 are PT_EINVAL too.
 *  - Kernels: the resume builds of variants 6, 10, 13 and 14; an automatic renderer gets the automatic policy's choice with
 *    8 and 9 replaced by 6.  pt_progressive_create refuses a renderer with an explicit other variant or fast_math.  Passes run
 *    unchunked.
 *  - A session shares its renderer's scratch (grid buffer, error word): do not run a session and its renderer concurrently on
 *    two streams (the same rule as for one denoiser's enqueues).  Passes are ordered after the renderer's last launch. */
typedef struct pt_progressive pt_progressive; /* opaque */
int pt_progressive_create(pt_renderer* r, pt_progressive** out);
int pt_progressive_reset(pt_progressive* p);
/* One pass of spp samples, asynchronous on hip_stream (NULL = default stream). */
int pt_progressive_enqueue(pt_progressive* p, int spp, float* d_out, const pt_sphere* d_spheres, int n_spheres,
                           const float basis[12], const float eye[3], void* hip_stream);
/* The same, synchronous on the default stream; *ms_out (may be NULL) = milliseconds between two device events around the pass. */
int pt_progressive_render(pt_progressive* p, int spp, float* d_out, const pt_sphere* d_spheres, int n_spheres,
                          const float basis[12], const float eye[3], float* ms_out);
int pt_progressive_samples(const pt_progressive* p, int64_t* samples);  /* samples per pixel so far */
int pt_progressive_variant(const pt_progressive* p, int n_spheres, int* variant);  /* the variant the next pass runs */
int pt_progressive_destroy(pt_progressive* p);

/* ---- adaptive sampling of a progressive session ------------------------------------------- */
/* Opt-in per session: pt_progressive_set_adaptive at 0 samples (after create or reset; later it is PT_EINVAL).  NULL turns it
 * off.  A session without the call behaves exactly as above.
 *  - Options: tolerance >= 0, the target relative standard error of a pixel's mean luminance; floor > 0, the luminance floor
 *    (dark pixels do not need infinitely many samples); min_samples >= 2, no pixel stops before this count; radius 0..4, the
 *    dilation window.  Any other value (NaN included) is PT_EINVAL.
 *  - Monotone active set.  The first pass renders every pixel.  Each later pass first decides which pixels stay active, then
 *    adds spp samples to exactly those.  A stopped pixel never resumes, so all active pixels hold the same count: the
 *    session's total (the sample index of a pass stays uniform across its launch).
 *  - Rule, for each pixel active in the last pass once the session holds n >= min_samples: with the pixel's frame values at n
 *    as the frame forms them (c0..c2 = sum / (float)n, c10 = the colour's Welford variance, lum = the reference's luminance of
 *    c0..c2), the pixel is CONVERGED when (a) no sample hit anything (depth 0), or (b) every one of its n samples scored
 *    (the colour variance skips escaped paths, pathtrace.cu:157-161) and
 *        (double)c10 <= ((double)tol * (double)tol * (double)n) * (m * m),  m = max((double)lum, (double)floor),
 *    evaluated left to right in double, with max as C's (double)lum > (double)floor ? lum : floor.  Two consequences for
 *    values that are not numbers: a NaN luminance takes the floor (the comparison is false), and a NaN variance never
 *    converges (it compares false against every threshold).  Because of the "every sample scored" condition, a pixel where some path escapes
 *    keeps sampling: adaptivity mostly helps closed scenes.
 *  - Dilation: a pixel stays active if it was active and an active, unconverged pixel lies in the (2 radius + 1)^2 window
 *    around it, clipped to the renderer's tile.
 *  - Every pass writes the WHOLE frame into d_out (pixels that stopped earlier included; d_out stays output only).  A pass
 *    with no active pixel adds nothing and only writes the frame.
 *  - Contract: after any pass, every pixel p with count n_p >= 2 is bit for bit pixel p of a fresh renderer's first Render()
 *    at n_p spp (the one-sample jitter exception above stays as it is).
 *  - pt_progressive_samples returns the maximum per-pixel count (synchronous for an adaptive session); the INT_MAX limit
 *    applies to the session's total, which is that maximum while any pixel is active.  pt_progressive_reset returns to 0
 *    samples with every pixel active and keeps the options.
 *  - Device memory: 9 bytes per tile pixel (count, list slot, mask) on top of the session's record, allocated by the first
 *    pt_progressive_set_adaptive call with options. */
typedef struct pt_adaptive_opts {
  float tolerance;      /* target relative standard error of the mean luminance, >= 0 */
  float floor;          /* luminance floor, > 0 */
  int32_t min_samples;  /* >= 2 */
  int32_t radius;       /* 0..4 */
} pt_adaptive_opts;
int pt_progressive_set_adaptive(pt_progressive* p, const pt_adaptive_opts* opts);
/* Synchronous: how many pixels the next pass renders (the whole tile for a plain session and before a first pass). */
int pt_progressive_active(pt_progressive* p, int64_t* active);
/* Every tile pixel's sample count (uint32, tile order) into device memory, device to device on hip_stream; a plain session's
 * counts are all its total. */
int pt_progressive_counts(pt_progressive* p, uint32_t* d_counts, void* hip_stream);

/* ---- host-side inputs of the path ------------------------------------------------------ */
/* The 9 spheres Scene() hard-codes, include/Scene.h:26-34 (host array). */
int pt_scene_cornell(pt_sphere out[9]);
/* Seeded random-sphere scene for BASELINE.json config 4 (no reference counterpart):
 * n spheres inside the Cornell box volume; with_walls != 0 appends nothing but makes the
 * first 6 entries the wall spheres of Scene.h:26-31 and the 7th the light (closed scene). */
int pt_scene_random(int n, uint64_t seed, int with_walls, pt_sphere* out);
/* Camera::updateCameraVectors + Camera::getEyeRayBasis, include/Camera.h:125-149,153-164,
 * restated without glm (float32, same operation order as glm 0.9.8). */
int pt_camera_basis(const float pos[3], float yaw_deg, float pitch_deg, int width, int height,
                    float basis_out[12]);
/* Same with an explicit WorldUp: the scalar constructor Camera(posX, posY, posZ, upX, upY, upZ, yaw, pitch),
 * include/Camera.h:63-70 (pt_camera_basis uses the (0, 1, 0) of the vector constructor, Camera.h:58). */
int pt_camera_basis_up(const float pos[3], float yaw_deg, float pitch_deg, const float world_up[3],
                       int width, int height, float basis_out[12]);

#ifdef __cplusplus
}
#endif
#endif /* PTCORE_H */
