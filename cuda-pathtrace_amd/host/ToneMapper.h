// ToneMapper.h -- RAII wrapper of pt_tonemap_* (include/ptcore.h): the stage between a frame of linear radiance and a picture.
// A metered exposure that stays on the device and adapts from frame to frame, a tone curve (clamp, Reinhard, ACES fit) and the
// correctly rounded sRGB encode; the result is RGBA8, one unsigned int per pixel.  The reference has no counterpart: its display
// path is Denoiser.h's clamp.  Shaped like TemporalAccumulator.h.  Errors print the GPUassert line and exit, like every
// look-alike class.
#ifndef TONEMAPPER_H
#define TONEMAPPER_H
#include <stddef.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "HipErrorCheck.h"
#include "OutputBuffer.h"

class ToneMapper {
 private:
  pt_tonemap* session;
  int width, height;
  unsigned int* d_rgba8;  // [height][width], owned
  ToneMapper(const ToneMapper&);
  ToneMapper& operator=(const ToneMapper&);

 public:
  static pt_tonemap_opts Defaults() {
    pt_tonemap_opts o;
    pt_tonemap_opts_default(&o);
    return o;
  }
  // opts: curve, encode, exposure (0 = auto), key, white, adapt (pt_tonemap_opts)
  ToneMapper(int width, int height, const pt_tonemap_opts& opts = Defaults()) : session(NULL), width(width), height(height), d_rgba8(NULL) {
    gpuErrchk(pt_tonemap_create(width, height, &opts, &session));
    gpuErrchk(pt_malloc((void**)&d_rgba8, (size_t)width * height * sizeof(unsigned int)));
  }
  ~ToneMapper() {
    (void)pt_tonemap_destroy(session);
    if (d_rgba8) (void)pt_free(d_rgba8);
  }

  // the device frame that Render() (and the accumulator, the filter or the network) left in d_buffer -> the session's RGBA8
  // image; the frame is not written; returns device-event milliseconds
  float Map(const OutputBuffer& d_buffer) {
    float ms = 0.0f;
    gpuErrchk(pt_tonemap_run(session, d_buffer.buffer, 14, d_rgba8, &ms));
    return ms;
  }
  // asynchronous on a HIP stream (NULL = default); pixelStride 14: a frame, 3: a filter's or denoiser's rgb image
  void Enqueue(const float* d_src, int pixelStride, unsigned int* d_out, void* hip_stream) {
    gpuErrchk(pt_tonemap_enqueue(session, d_src, pixelStride, d_out, hip_stream));
  }
  // the scene was cut: the next frame's exposure is its own target
  void Reset() { gpuErrchk(pt_tonemap_reset(session)); }
  // waits for the device
  float Exposure() {
    float e = 0.0f;
    gpuErrchk(pt_tonemap_exposure(session, &e));
    return e;
  }

  // the last mapped image as a binary PPM (P6); false when the file cannot be written
  bool SavePPM(const std::string& path) {
    std::vector<unsigned int> rgba((size_t)width * height);
    gpuErrchk(pt_memcpy_d2h(rgba.data(), d_rgba8, rgba.size() * sizeof(unsigned int)));
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < rgba.size(); i++) {
      const unsigned char rgb[3] = {(unsigned char)(rgba[i] & 255u), (unsigned char)((rgba[i] >> 8) & 255u),
                                    (unsigned char)((rgba[i] >> 16) & 255u)};
      fwrite(rgb, 1, 3, f);
    }
    return fclose(f) == 0;
  }
};
#endif
