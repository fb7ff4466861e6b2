// pt_internal.h -- error plumbing shared by the host-side translation units of libptcore.
#pragma once
#include "../../include/ptcore.h"

// Records `msg` (printf-style) as the calling thread's last error and returns `code`.
int pt_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Returns from the calling function with the HIP error of `call` as the last error: PT_ENODEVICE when no device is there,
// PT_EHIP otherwise.  (For translation units that include <hip/hip_runtime.h>.)
#define PT_HIP(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return pt_fail(e_ == hipErrorNoDevice ? PT_ENODEVICE : PT_EHIP, "%s: %s (%s:%d)", #call,    \
                     hipGetErrorString(e_), __FILE__, __LINE__);                                  \
  } while (0)

// The same for the display packer and the lab diagnostics, which never report PT_ENODEVICE: every error is PT_EHIP.
#define PT_HIPD(call)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) return pt_fail(PT_EHIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
