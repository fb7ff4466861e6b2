// DenoiseNet.h -- RAII wrapper of pt_denoiser_* (include/ptcore.h): the reference's denoising network, DenoiseCNN
// (denoise_cnn/model.py), which its interactive loop runs on the frame tensor after every Render() through
// train.py:test() (src/main.cu:92-122,146-152).  Not to be confused with Denoiser.h, the reference's display packer.
// Errors print the GPUassert line and exit, like every look-alike class.
#ifndef DENOISENET_H
#define DENOISENET_H
#include <stddef.h>

#include <string>

#include "HipErrorCheck.h"
#include "OutputBuffer.h"

class DenoiseNet {
 private:
  pt_denoiser* net;
  int width, height;
  DenoiseNet(const DenoiseNet&);
  DenoiseNet& operator=(const DenoiseNet&);

 public:
  // load_pretrained + .eval() for width x height frames; weights = a PTDN file (cuda-pathtrace_amd/denoise_weights.py).
  // maxFrames > 1: workspace for batches of that many frames per group (DenoiseFrames / EnqueueFrames).
  // precision: PT_DENOISE_F32 (default) or PT_DENOISE_F16, the toleranced half mode (fp16 operands and storage, fp32
  // accumulation; include/ptcore.h states its contract).
  DenoiseNet(int width, int height, const std::string& weights, int maxFrames = 1, int precision = PT_DENOISE_F32)
      : net(NULL), width(width), height(height) {
    pt_denoiser_opts opts = pt_denoiser_opts();
    opts.precision = precision;
    opts.max_frames = maxFrames;
    gpuErrchk(pt_denoiser_create_opts_from_file(width, height, weights.c_str(), &opts, &net));
  }
  int Precision() const {
    int p = PT_DENOISE_F32;
    gpuErrchk(pt_denoiser_precision(net, &p));
    return p;
  }
  ~DenoiseNet() { (void)pt_denoiser_destroy(net); }

  // train.py:test + modify_tensor (main.cu:106,150-152): in place on the device frame; returns device-event milliseconds
  float Denoise(OutputBuffer& d_buffer) {
    float ms = 0.0f;
    gpuErrchk(pt_denoiser_denoise(net, d_buffer.buffer, NULL, &ms));
    return ms;
  }
  // asynchronous on a HIP stream (NULL = default); d_rgb != NULL: [H][W][3] result there, frame untouched
  void Enqueue(float* d_frame, float* d_rgb, void* hip_stream) { gpuErrchk(pt_denoiser_enqueue(net, d_frame, d_rgb, hip_stream)); }

  // n device frames strideFloats apart (e.g. the buffer of Renderer::RenderFrames), each in place, bit for bit n Denoise
  // calls; returns device-event milliseconds for all of them
  float DenoiseFrames(float* d_frames, int n, size_t strideFloats) {
    float ms = 0.0f;
    gpuErrchk(pt_denoiser_denoise_frames(net, n, d_frames, strideFloats, NULL, 0, &ms));
    return ms;
  }
  // asynchronous batch; d_rgb != NULL: [H][W][3] results rgbStrideFloats apart, frames untouched
  void EnqueueFrames(float* d_frames, int n, size_t strideFloats, float* d_rgb, size_t rgbStrideFloats, void* hip_stream) {
    gpuErrchk(pt_denoiser_enqueue_frames(net, n, d_frames, strideFloats, d_rgb, rgbStrideFloats, hip_stream));
  }
};
#endif
