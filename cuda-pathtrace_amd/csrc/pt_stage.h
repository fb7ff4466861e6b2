// pt_stage.h -- the host scaffold of a post-process stage session (pt_denoise.hip, pt_filter.hip, pt_temporal.hip,
// pt_tonemap.hip, pt_compare.hip, pt_patches.hip): the checks, the timed run, the workspace growth and the create / destroy tail that every stage needs and
// none should spell out again.  Host code only; a stage keeps its own plain struct (with `hipEvent_t ev0, ev1`), its option
// checks, its check_args, its launch loops and its kernels.  Every helper takes the caller's `who` for the message.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "pt_internal.h"

namespace pt_stage {

// The limits of a group of frames: gridDim.y / .z of the per-frame kernels, and every pixel index of a group inside int32.
constexpr int MAX_FRAMES = 65535;
constexpr int64_t MAX_BATCH_PIXELS = (int64_t)1 << 26;

inline bool finite_f(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }

inline int check_frame_size(const char* who, int width, int height) {
  if (width <= 0 || width > 16384) return pt_fail(PT_EINVAL, "%s: width %d outside 1 .. 16384", who, width);
  if (height <= 0 || height > 16384) return pt_fail(PT_EINVAL, "%s: height %d outside 1 .. 16384", who, height);
  if ((int64_t)width * height > 4096 * 4096)
    return pt_fail(PT_EINVAL, "%s: frame size %d x %d (width x height) exceeds 4096 x 4096 pixels", who, width, height);
  return PT_OK;
}

inline int check_batch(const char* who, int max_frames, int width, int height) {
  if (max_frames > MAX_FRAMES || (int64_t)max_frames * width * height > MAX_BATCH_PIXELS)
    return pt_fail(PT_EINVAL, "%s: max_frames %d x %d x %d pixels exceeds the limit of %d frames and %lld pixels", who, max_frames, width,
                   height, MAX_FRAMES, (long long)MAX_BATCH_PIXELS);
  return PT_OK;
}

// The last refusal of a create, after every check of its arguments: nothing runs without a device.
inline int check_device(const char* who) {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice || (e == hipSuccess && n == 0))
    return pt_fail(PT_ENODEVICE, "%s: no HIP device visible (there is no CPU fallback)", who);
  if (e != hipSuccess) return pt_fail(PT_EHIP, "%s: hipGetDeviceCount: %s (no usable device)", who, hipGetErrorString(e));
  return PT_OK;
}

// `enqueue()` on the null stream between the two events; the kernel time goes to *ms_out unless that is null.  The caller has
// checked its arguments: a refused call must not touch the device.
template <class Enqueue>
int run_timed(hipEvent_t ev0, hipEvent_t ev1, float* ms_out, Enqueue enqueue) {
  PT_HIP(hipEventRecord(ev0, nullptr));
  const int rc = enqueue();
  if (rc != PT_OK) return rc;
  PT_HIP(hipEventRecord(ev1, nullptr));
  PT_HIP(hipEventSynchronize(ev1));
  float ms = 0.0f;
  PT_HIP(hipEventElapsedTime(&ms, ev0, ev1));
  if (ms_out) *ms_out = ms;
  return PT_OK;
}

// One device buffer of a session's workspace: where the session keeps its pointer, its new size (0: none, the pointer
// becomes null) and whether the new buffer starts as zeros.
struct Buffer {
  void** slot;
  size_t bytes;
  bool zeroed;
};

// Replaces the N buffers by new ones of the given sizes.  All of the new ones first, then a wait for the work that may still
// use the old ones; a failure frees what it got, clears HIP's last error and leaves the session as it was.  `asked` (printf
// style) is the caller's wording of what it asked for.
template <int N>
__attribute__((format(printf, 3, 4))) int grow_workspace(const char* who, const Buffer (&bufs)[N], const char* asked, ...) {
  void* grown[N] = {};
  hipError_t e = hipSuccess;
  for (int i = 0; i < N; i++) {
    if (e == hipSuccess && bufs[i].bytes) e = hipMalloc(&grown[i], bufs[i].bytes);
    if (e == hipSuccess && bufs[i].bytes && bufs[i].zeroed) e = hipMemset(grown[i], 0, bufs[i].bytes);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipGetLastError();
    for (void* p : grown)
      if (p) (void)hipFree(p);
    char text[128];
    va_list ap;
    va_start(ap, asked);
    vsnprintf(text, sizeof(text), asked, ap);
    va_end(ap);
    return pt_fail(PT_EHIP, "%s: %s: %s; the old workspace is kept", who, text, hipGetErrorString(e));
  }
  for (int i = 0; i < N; i++) {
    if (*bufs[i].slot) (void)hipFree(*bufs[i].slot);
    *bufs[i].slot = grown[i];
  }
  return PT_OK;
}

// The tail of a create: `e` is the outcome of the stage's own allocations, the two events follow.  On an error the session
// goes back through the stage's destroy.
template <class Session>
int create_events(const char* who, hipError_t e, Session* s, int (*destroy)(Session*)) {
  if (e == hipSuccess) e = hipEventCreate(&s->ev0);
  if (e == hipSuccess) e = hipEventCreate(&s->ev1);
  if (e == hipSuccess) return PT_OK;
  const int rc = pt_fail(e == hipErrorNoDevice ? PT_ENODEVICE : PT_EHIP, "%s: %s", who, hipGetErrorString(e));
  destroy(s);
  return rc;
}

template <class Session>
void destroy_events(Session* s) {
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
}

}  // namespace pt_stage
