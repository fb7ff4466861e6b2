// PatchSampler.h -- RAII wrapper of pt_patches_* (include/ptcore.h): from the 2-spp frame and its converged twin, both in device
// buffers, the pre-processed [N][14][P][P] inputs and clamped [N][3][P][P] targets a denoiser is trained on, and the score by
// which the reference chooses its patches -- what denoise_cnn/load_data.py computes off the device, with the pre-processing
// Denoiser applies at inference, bit for bit.  Neither frame is written.  The product of this stage is tensors, for which the
// command line has no format: there is no flag of `pathtrace` for it.  Shaped like FrameCompare.h.  Errors print the GPUassert
// line and exit, like every look-alike class.
#ifndef PATCHSAMPLER_H
#define PATCHSAMPLER_H
#include <stddef.h>
#include <stdint.h>

#include "HipErrorCheck.h"
#include "OutputBuffer.h"

class PatchSampler {
 private:
  pt_patches* session;
  int patch, maxPatches;
  PatchSampler(const PatchSampler&);
  PatchSampler& operator=(const PatchSampler&);

 public:
  PatchSampler(int width, int height, int patch, int maxPatches = 64) : session(NULL), patch(patch), maxPatches(maxPatches) {
    pt_patches_opts opts;
    pt_patches_opts_default(&opts);
    opts.patch = patch;
    opts.max_patches = maxPatches;
    gpuErrchk(pt_patches_create(width, height, &opts, &session));
  }
  ~PatchSampler() { (void)pt_patches_destroy(session); }

  int Patch() const { return patch; }
  int MaxPatches() const { return maxPatches; }  // the most corners of one Score or Gather
  // floats of the inputs / targets of n patches
  size_t InputFloats(int n) const { return (size_t)n * 14 * patch * patch; }
  size_t TargetFloats(int n) const { return (size_t)n * 3 * patch * patch; }

  // the divisors of the frame that Render() left in d_train: once per frame, before Score and Gather of that frame
  void Prepare(const OutputBuffer& d_train, void* hip_stream = NULL) { gpuErrchk(pt_patches_prepare(session, d_train.buffer, hip_stream)); }
  // corners: n host (x, y) pairs, free again when the call returns; asynchronous on a HIP stream (NULL = default)
  void Score(const OutputBuffer& d_train, int n, const int32_t* corners, void* hip_stream = NULL) {
    gpuErrchk(pt_patches_score(session, d_train.buffer, n, corners, hip_stream));
  }
  // waits for the device: the sums and the score of patch k of the last Score
  pt_patches_values Result(int k) {
    pt_patches_values v;
    gpuErrchk(pt_patches_result(session, k, &v));
    return v;
  }
  // d_inputs: InputFloats(n) device floats; d_targets: TargetFloats(n), from the converged frame d_gt, or NULL
  void Gather(const OutputBuffer& d_train, const OutputBuffer& d_gt, int n, const int32_t* corners, float* d_inputs, float* d_targets,
              void* hip_stream = NULL) {
    gpuErrchk(pt_patches_gather(session, d_train.buffer, d_gt.buffer, 14, n, corners, d_inputs, d_targets, hip_stream));
  }
};
#endif
