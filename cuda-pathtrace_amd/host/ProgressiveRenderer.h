// ProgressiveRenderer.h -- RAII wrapper of pt_progressive_* (include/ptcore.h): one still frame of a Renderer refined pass by
// pass.  The reference's interactive loop renders a resting camera's frame again from fresh samples every iteration
// (src/main.cu:146-177, pathtrace.cu:212-256); Refine() adds samples to the same frame instead.  After a pass that leaves the
// session at n >= 2 samples the buffer holds exactly the frame a fresh Renderer's first Render() at n spp writes.
// Errors print the GPUassert line and exit, like every look-alike class.
#ifndef PROGRESSIVERENDERER_H
#define PROGRESSIVERENDERER_H
#include "Camera.h"
#include "HipErrorCheck.h"
#include "OutputBuffer.h"
#include "Renderer.h"
#include "Scene.h"

class ProgressiveRenderer {
 private:
  pt_progressive* session;
  int width, height;
  ProgressiveRenderer(const ProgressiveRenderer&);
  ProgressiveRenderer& operator=(const ProgressiveRenderer&);

 public:
  // the session shares the renderer's scratch: do not render with both at once on two streams; the renderer must outlive it
  ProgressiveRenderer(Renderer& renderer, int width, int height) : session(NULL), width(width), height(height) {
    gpuErrchk(pt_progressive_create(renderer.Handle(), &session));
  }
  ~ProgressiveRenderer() { (void)pt_progressive_destroy(session); }

  // spp more samples per pixel; d_buffer receives the frame of all samples so far.  Synchronous, returns device-event
  // milliseconds like Renderer::Render.  The camera and scene must be those of the session's first pass (else: Reset()).
  float Refine(OutputBuffer d_buffer, const Scene& d_scene, const Camera& camera, int spp) {
    float3 eyeRayBasis[4];
    camera.getEyeRayBasis(eyeRayBasis, width, height);
    float basis[12], eye[3] = {camera.Position.x, camera.Position.y, camera.Position.z};
    for (int k = 0; k < 4; k++) {
      basis[3 * k] = eyeRayBasis[k].x;
      basis[3 * k + 1] = eyeRayBasis[k].y;
      basis[3 * k + 2] = eyeRayBasis[k].z;
    }
    float milliseconds = 0;
    gpuErrchk(pt_progressive_render(session, spp, d_buffer.buffer, reinterpret_cast<const pt_sphere*>(d_scene.objects),
                                    d_scene.numObjects, basis, eye, &milliseconds));
    return milliseconds;
  }
  long long Samples() {
    int64_t n = 0;
    gpuErrchk(pt_progressive_samples(session, &n));
    return (long long)n;
  }
  void Reset() { gpuErrchk(pt_progressive_reset(session)); }

  // Adaptive sampling (include/ptcore.h, pt_progressive_set_adaptive): only at 0 samples; later passes render only the pixels
  // whose mean luminance is not yet within `tolerance` (relative standard error).  Samples() is then the maximum count.
  void SetAdaptive(float tolerance, float floor, int minSamples, int radius) {
    pt_adaptive_opts o;
    o.tolerance = tolerance;
    o.floor = floor;
    o.min_samples = minSamples;
    o.radius = radius;
    gpuErrchk(pt_progressive_set_adaptive(session, &o));
  }
  // how many pixels the next Refine() renders (synchronous)
  long long Active() {
    int64_t n = 0;
    gpuErrchk(pt_progressive_active(session, &n));
    return (long long)n;
  }
  // every pixel's sample count into d_counts (width * height uint32 in device memory, row-major); synchronous
  void Counts(unsigned int* d_counts) {
    gpuErrchk(pt_progressive_counts(session, d_counts, NULL));
    gpuErrchk(pt_device_synchronize());
  }
};
#endif
