// TemporalAccumulator.h -- RAII wrapper of pt_temporal_* (include/ptcore.h): the temporal stage in front of FeatureFilter.h.
// Every frame of a fly-through is reprojected into the previous frame's camera through its own depth channel and blended with
// what the earlier frames accumulated there; the count image it writes is what FeatureFilter::Filter takes as d_counts.  The
// reference has no counterpart.  Shaped like FeatureFilter.h.  Errors print the GPUassert line and exit, like every look-alike
// class.
#ifndef TEMPORALACCUMULATOR_H
#define TEMPORALACCUMULATOR_H
#include <stddef.h>

#include "Camera.h"
#include "HipErrorCheck.h"
#include "OutputBuffer.h"
#include "Scene.h"

class TemporalAccumulator {
 private:
  pt_temporal* session;
  int width, height;
  TemporalAccumulator(const TemporalAccumulator&);
  TemporalAccumulator& operator=(const TemporalAccumulator&);

 public:
  static pt_temporal_opts Defaults() {
    pt_temporal_opts o;
    pt_temporal_opts_default(&o);
    return o;
  }
  // opts: the history cap in samples and the four stops (pt_temporal_opts)
  TemporalAccumulator(int width, int height, const pt_temporal_opts& opts = Defaults()) : session(NULL), width(width), height(height) {
    gpuErrchk(pt_temporal_create(width, height, &opts, &session));
  }
  ~TemporalAccumulator() { (void)pt_temporal_destroy(session); }

  // in place on the device frame that Render() produced with `camera` at `samples` samples per pixel; d_counts != NULL: the
  // accumulated per-pixel counts (unsigned int [height][width]) for FeatureFilter::Filter; returns device-event milliseconds
  float Accumulate(OutputBuffer& d_buffer, int samples, const Camera& camera, unsigned int* d_counts = NULL) {
    float basis[12], eye[3];
    Pose(camera, basis, eye);
    float ms = 0.0f;
    gpuErrchk(pt_temporal_run(session, d_buffer.buffer, samples, basis, eye, d_counts, &ms));
    return ms;
  }
  // the same for an animated scene: `scene` holds the HOST spheres the frame was rendered from.  The session remembers them,
  // and from the second call on every pixel follows the sphere its centre ray hits (pt_temporal_run_scene): spheres may move
  // between calls by rigid translation; a sphere count or a radius that changes exits like every error -- Reset() first.
  float Accumulate(OutputBuffer& d_buffer, int samples, const Camera& camera, const std::vector<Sphere>& scene, unsigned int* d_counts = NULL) {
    float basis[12], eye[3];
    Pose(camera, basis, eye);
    float ms = 0.0f;
    gpuErrchk(pt_temporal_run_scene(session, d_buffer.buffer, samples, basis, eye, reinterpret_cast<const pt_sphere*>(scene.data()),
                                    (int)scene.size(), d_counts, &ms));
    return ms;
  }
  // asynchronous on a HIP stream (NULL = default)
  void Enqueue(float* d_frame, int samples, const Camera& camera, unsigned int* d_counts, void* hip_stream) {
    float basis[12], eye[3];
    Pose(camera, basis, eye);
    gpuErrchk(pt_temporal_enqueue(session, d_frame, samples, basis, eye, d_counts, hip_stream));
  }
  // the scene changed: the next frame passes through
  void Reset() { gpuErrchk(pt_temporal_reset(session)); }
  // the responsive history (pt_temporal_set_antilag): a second history of at most fast_cap samples, and after every Accumulate
  // the long history's colour is clamped into mu +- sigma standard deviations of the fast colours in the (2 radius + 1)^2 window
  // around the pixel, so that shadows and indirect light of moving spheres do not lag.  fast_cap 0 switches it off.  Only before
  // the first frame or right after Reset(); a bad value exits like every error.
  void SetAntilag(float fast_cap, float sigma = PT_ANTILAG_DEFAULT_SIGMA, int radius = PT_ANTILAG_DEFAULT_RADIUS) {
    pt_temporal_antilag_opts o;
    pt_temporal_antilag_opts_default(&o);
    o.fast_cap = fast_cap, o.clamp_sigma = sigma, o.clamp_radius = radius;
    gpuErrchk(pt_temporal_set_antilag(session, &o));
  }
  // debug view: the fast image the last Accumulate wrote, [height][width][4] floats {fast rgb, fast count}, into d_out
  void Fast(float* d_out, void* hip_stream = NULL) { gpuErrchk(pt_temporal_fast(session, d_out, hip_stream)); }

 private:
  void Pose(const Camera& camera, float basis[12], float eye[3]) const {
    float3 eyeRayBasis[4];
    camera.getEyeRayBasis(eyeRayBasis, width, height);  // as Renderer::Render
    for (int k = 0; k < 4; k++) {
      basis[3 * k] = eyeRayBasis[k].x;
      basis[3 * k + 1] = eyeRayBasis[k].y;
      basis[3 * k + 2] = eyeRayBasis[k].z;
    }
    eye[0] = camera.Position.x, eye[1] = camera.Position.y, eye[2] = camera.Position.z;
  }
};
#endif
