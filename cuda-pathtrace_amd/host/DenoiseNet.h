// DenoiseNet.h -- RAII wrapper of pt_denoiser_* (include/ptcore.h): the reference's denoising network, DenoiseCNN
// (denoise_cnn/model.py), which its interactive loop runs on the frame tensor after every Render() through
// train.py:test() (src/main.cu:92-122,146-152).  Not to be confused with Denoiser.h, the reference's display packer.
// Errors print the GPUassert line and exit, like every look-alike class.
#ifndef DENOISENET_H
#define DENOISENET_H
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
  // load_pretrained + .eval() for width x height frames; weights = a PTDN file (cuda-pathtrace_amd/denoise_weights.py)
  DenoiseNet(int width, int height, const std::string& weights) : net(NULL), width(width), height(height) {
    gpuErrchk(pt_denoiser_create_from_file(width, height, weights.c_str(), &net));
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
};
#endif
