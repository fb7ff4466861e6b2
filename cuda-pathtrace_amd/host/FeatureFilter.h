// FeatureFilter.h -- RAII wrapper of pt_filter_* (include/ptcore.h): the weights-free denoiser, a variance-guided edge-avoiding
// a-trous filter on albedo-demodulated colour driven by the frame's own normal, albedo, depth and variance channels
// (src/pathtrace.cu:240-254 writes them).  The reference has no counterpart: its only denoiser is the CNN of DenoiseNet.h,
// for which it ships no weights.  Shaped like DenoiseNet.h.  Errors print the GPUassert line and exit, like every look-alike class.
#ifndef FEATUREFILTER_H
#define FEATUREFILTER_H
#include <stddef.h>

#include "HipErrorCheck.h"
#include "OutputBuffer.h"

class FeatureFilter {
 private:
  pt_filter* filter;
  int width, height;
  FeatureFilter(const FeatureFilter&);
  FeatureFilter& operator=(const FeatureFilter&);

 public:
  static pt_filter_opts Defaults() {
    pt_filter_opts o;
    pt_filter_opts_default(&o);
    return o;
  }
  // opts: iterations 1 .. 8 and the four stops (pt_filter_opts); opts.max_frames > 1: workspace for batches of that many
  // frames per group (FilterFrames / EnqueueFrames)
  FeatureFilter(int width, int height, const pt_filter_opts& opts = Defaults()) : filter(NULL), width(width), height(height) {
    gpuErrchk(pt_filter_create(width, height, &opts, &filter));
  }
  ~FeatureFilter() { (void)pt_filter_destroy(filter); }
  // the spatial variance estimate (pt_filter_set_spatial): before the first iteration every pixel with fewer than `below`
  // samples takes the larger of its own variance and the spread of its neighbours' luminances on the same surface, over the
  // (2 radius + 1)^2 window.  below 0 switches it off, PT_FILTER_SPATIAL_ALL takes every pixel; it holds for every later
  // call.  A bad value exits like every error.
  void SetSpatial(unsigned int below, int radius = PT_FILTER_SPATIAL_DEFAULT_RADIUS) {
    pt_filter_spatial_opts o;
    pt_filter_spatial_opts_default(&o);
    o.below = below, o.radius = radius;
    gpuErrchk(pt_filter_set_spatial(filter, &o));
  }

  // in place on the device frame rendered with `samples` samples per pixel (d_counts != NULL: the per-pixel counts of an
  // adaptive session instead); returns device-event milliseconds
  float Filter(OutputBuffer& d_buffer, int samples, const unsigned int* d_counts = NULL) {
    float ms = 0.0f;
    gpuErrchk(pt_filter_run(filter, d_buffer.buffer, NULL, samples, d_counts, &ms));
    return ms;
  }
  // asynchronous on a HIP stream (NULL = default); d_rgb != NULL: [H][W][3] result there, frame untouched
  void Enqueue(float* d_frame, float* d_rgb, int samples, const unsigned int* d_counts, void* hip_stream) {
    gpuErrchk(pt_filter_enqueue(filter, d_frame, d_rgb, samples, d_counts, hip_stream));
  }

  // n device frames strideFloats apart (e.g. the buffer of Renderer::RenderFrames), each in place, bit for bit n Filter
  // calls; returns device-event milliseconds for all of them
  float FilterFrames(float* d_frames, int n, size_t strideFloats, int samples) {
    float ms = 0.0f;
    gpuErrchk(pt_filter_run_frames(filter, n, d_frames, strideFloats, NULL, 0, samples, &ms));
    return ms;
  }
  // asynchronous batch; d_rgb != NULL: [H][W][3] results rgbStrideFloats apart, frames untouched
  void EnqueueFrames(float* d_frames, int n, size_t strideFloats, float* d_rgb, size_t rgbStrideFloats, int samples, void* hip_stream) {
    gpuErrchk(pt_filter_enqueue_frames(filter, n, d_frames, strideFloats, d_rgb, rgbStrideFloats, samples, hip_stream));
  }
  void ReserveFrames(int n) { gpuErrchk(pt_filter_reserve_frames(filter, n)); }
};
#endif
