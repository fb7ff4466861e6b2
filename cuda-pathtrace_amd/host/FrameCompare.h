// FrameCompare.h -- RAII wrapper of pt_compare_* (include/ptcore.h): how far the frame in a device buffer is from a reference
// picture -- clamped MSE (rms, psnr), capped relMSE and SSIM, measured on the device in one pass over both.  The session keeps the
// reference's colour on the device ([height][width][3]); a frame is never written.  The reference has no counterpart: it judges
// its 2-spp frames against its 20000-spp frames off the device.  Shaped like ToneMapper.h.  Errors print the GPUassert line and
// exit, like every look-alike class.
#ifndef FRAMECOMPARE_H
#define FRAMECOMPARE_H
#include <stddef.h>

#include <vector>

#include "HipErrorCheck.h"
#include "OutputBuffer.h"

class FrameCompare {
 private:
  pt_compare* session;
  int width, height;
  float* d_reference;  // [height][width][3], owned
  FrameCompare(const FrameCompare&);
  FrameCompare& operator=(const FrameCompare&);

 public:
  // reference: a host frame [height][width][14] (what ptexr::LoadFeatureEXR decodes); its colour goes to the device
  FrameCompare(int width, int height, const float* reference) : session(NULL), width(width), height(height), d_reference(NULL) {
    gpuErrchk(pt_compare_create(width, height, NULL, &session));
    std::vector<float> rgb((size_t)width * height * 3);
    for (size_t p = 0; p < (size_t)width * height; p++)
      for (int k = 0; k < 3; k++) rgb[p * 3 + k] = reference[p * 14 + k];
    gpuErrchk(pt_malloc((void**)&d_reference, rgb.size() * sizeof(float)));
    gpuErrchk(pt_memcpy_h2d(d_reference, rgb.data(), rgb.size() * sizeof(float)));
  }
  ~FrameCompare() {
    (void)pt_compare_destroy(session);
    if (d_reference) (void)pt_free(d_reference);
  }

  // the device frame that Render() (and the accumulator, the filter or the network) left in d_buffer against the reference;
  // returns device-event milliseconds
  float Compare(const OutputBuffer& d_buffer) {
    float ms = 0.0f;
    gpuErrchk(pt_compare_run(session, d_buffer.buffer, 14, d_reference, 3, NULL, &ms));
    return ms;
  }
  // asynchronous on a HIP stream (NULL = default); pixelStride 14: a frame, 3: an rgb image; d_map may be NULL
  void Enqueue(const float* d_img, int pixelStride, float* d_map, void* hip_stream) {
    gpuErrchk(pt_compare_enqueue(session, d_img, pixelStride, d_reference, 3, d_map, hip_stream));
  }
  // waits for the device: the sums and the values of the last comparison
  pt_compare_values Result() {
    pt_compare_values v;
    gpuErrchk(pt_compare_result(session, 0, &v));
    return v;
  }
};
#endif
