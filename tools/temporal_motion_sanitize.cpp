// temporal_motion_sanitize.cpp -- a stand-alone program (its own main, no device, no Python) that drives the host-side code of the
// moving-sphere calls under AddressSanitizer and UBSan: the scene checks of pt_temporal_scene_check on arrays of exactly n
// spheres (an over-read is an error), the null-session refusals of the motion calls, and the velocity list of
// `pathtrace --velocities` (host/Velocities.h) on good and bad files.  pt_temporal.hip is compiled into it unchanged; pt_fail and
// pt_last_error, which live in pt_capi.hip with the rest of the C ABI, are restated here in a few lines.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include -I cuda-pathtrace_amd/csrc \
//         tools/temporal_motion_sanitize.cpp cuda-pathtrace_amd/csrc/pt_temporal.hip -o /tmp/temporal_motion_sanitize
//   /tmp/temporal_motion_sanitize          # prints "temporal_motion_sanitize: N checks, 0 failed" and exits 0
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cuda-pathtrace_amd/host/Velocities.h"

static char g_err[512];
int pt_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char* pt_last_error(void) { return g_err; }

static int g_checks = 0, g_failed = 0;
static void expect(bool ok, const char* what) {
  g_checks++;
  if (!ok) {
    g_failed++;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
  }
}
static void refused(int rc, const char* word, const char* what) { expect(rc == PT_EINVAL && strstr(g_err, word) != NULL, what); }

static std::vector<pt_sphere> scene(int n) {
  std::vector<pt_sphere> s((size_t)n);
  for (int i = 0; i < n; i++) {
    s[(size_t)i].radius = 1.0f + (float)(i % 7);
    for (int k = 0; k < 3; k++) s[(size_t)i].pos[k] = (float)(i + k), s[(size_t)i].emission[k] = 0.0f, s[(size_t)i].color[k] = 0.5f;
  }
  return s;
}

static std::string write_file(const char* name, const char* text) {
  const std::string path = std::string("/tmp/temporal_motion_sanitize_") + name;
  FILE* f = fopen(path.c_str(), "w");
  if (f) {
    fputs(text, f);
    fclose(f);
  }
  return path;
}

int main() {
  const float basis[12] = {-0.5f, -0.25f, -1.0f, 1.5f, -0.25f, -1.0f, -0.5f, 0.75f, -1.0f, 1.5f, 0.75f, -1.0f};
  const float eye[3] = {50.0f, 52.0f, 295.5f};

  // ---- pt_temporal_scene_check: arrays of exactly n spheres on the heap
  for (int n : {1, 9, 255, 256, 257, 65535}) {
    std::vector<pt_sphere> now = scene(n), prev = scene(n);
    for (pt_sphere& s : prev) s.pos[0] -= 1.5f;
    expect(pt_temporal_scene_check(now.data(), prev.data(), n, basis, eye) == PT_OK, "a good pair of scenes");
    now[(size_t)n - 1].color[2] = NAN;
    refused(pt_temporal_scene_check(now.data(), prev.data(), n, basis, eye), "color[2]", "NaN in the last float of the array");
    now[(size_t)n - 1].color[2] = 0.5f;
    prev[(size_t)n - 1].radius = nextafterf(prev[(size_t)n - 1].radius, 100.0f);
    refused(pt_temporal_scene_check(now.data(), prev.data(), n, basis, eye), "reset the session", "a radius one ulp apart");
  }
  {
    std::vector<pt_sphere> s = scene(9);
    refused(pt_temporal_scene_check(s.data(), s.data(), 0, basis, eye), "n 0 outside", "n = 0");
    refused(pt_temporal_scene_check(s.data(), s.data(), -1, basis, eye), "outside", "n < 0");
    refused(pt_temporal_scene_check(s.data(), s.data(), 65536, basis, eye), "outside", "n too large is refused before the array is read");
    refused(pt_temporal_scene_check(NULL, s.data(), 9, basis, eye), "null h_now", "null h_now");
    refused(pt_temporal_scene_check(s.data(), NULL, 9, basis, eye), "null h_prev", "null h_prev");
    refused(pt_temporal_scene_check(s.data(), s.data(), 9, NULL, eye), "null basis", "null basis");
    refused(pt_temporal_scene_check(s.data(), s.data(), 9, basis, NULL), "null eye", "null eye");
    float flat[12];
    memcpy(flat, basis, sizeof(flat));
    for (int k = 0; k < 3; k++) flat[3 + k] = flat[k];
    refused(pt_temporal_scene_check(s.data(), s.data(), 9, flat, eye), "determinant", "a basis without width");
    const float bad_eye[3] = {50.0f, INFINITY, 0.0f};
    refused(pt_temporal_scene_check(s.data(), s.data(), 9, basis, bad_eye), "eye[1]", "an infinite eye");
    // the calls that need a session refuse a null one before anything else
    refused(pt_temporal_motion(NULL, s.data(), s.data(), 9, basis, eye, NULL, NULL), "null accumulator", "pt_temporal_motion");
    refused(pt_temporal_enqueue_motion(NULL, NULL, 4, basis, eye, NULL, NULL, NULL), "null accumulator", "pt_temporal_enqueue_motion");
    refused(pt_temporal_run_motion(NULL, NULL, 4, basis, eye, NULL, NULL, NULL), "null accumulator", "pt_temporal_run_motion");
    refused(pt_temporal_enqueue_scene(NULL, NULL, 4, basis, eye, s.data(), 9, NULL, NULL), "null accumulator", "pt_temporal_enqueue_scene");
    refused(pt_temporal_run_scene(NULL, NULL, 4, basis, eye, s.data(), 9, NULL, NULL), "null accumulator", "pt_temporal_run_scene");
    refused(pt_temporal_enqueue_frames_scenes(NULL, 2, NULL, 14, basis, eye, s.data(), 9, 4, NULL, NULL), "null accumulator", "frames_scenes");
    refused(pt_temporal_run_frames_scenes(NULL, 2, NULL, 14, basis, eye, s.data(), 9, 4, NULL, NULL), "null accumulator", "run_frames_scenes");
  }

  // ---- the velocity list
  {
    std::vector<SphereVelocity> v;
    std::string why;
    expect(ParseVelocities(write_file("good", "# two spheres\n7 2.5 0 1\n\n 8\t-1e-3 0.125 3 \r\n"), 9, v, why) && v.size() == 2 && v[1].index == 8 &&
               v[0].v[0] == 2.5f && v[1].v[1] == 0.125f,
           "a good list");
    const char* bad[][2] = {{"9 1 0 0\n", "outside"},      {"-1 1 0 0\n", "outside"}, {"7 1 0 0\n7 1 0 0\n", "repeated"}, {"7 nan 0 0\n", "finite"},
                            {"7 0 -inf 0\n", "finite"},    {"7 0 0 1e39\n", "finite"}, {"7 1 0\n", "expected"},            {"7 1 0 0 0\n", "expected"},
                            {"7 1x 0 0\n", "expected"},    {"x 1 0 0\n", "expected"},  {"", "no velocities"},              {"#\n\n", "no velocities"},
                            {"99999999999999999999 1 0 0\n", "expected"}, {"7.5 1 0\n", "expected"}, {"7.5 1 0 0\n", "expected"}};
    for (auto& b : bad) expect(!ParseVelocities(write_file("bad", b[0]), 9, v, why) && why.find(b[1]) != std::string::npos, b[0]);
    expect(!ParseVelocities("/tmp/temporal_motion_sanitize_no_such_file", 9, v, why) && why.find("cannot open") != std::string::npos, "no file");
    expect(!ParseVelocities(write_file("zero", "0 1 0 0\n"), 0, v, why), "a scene without spheres has no index");

    std::vector<Sphere> at0(9), now;
    for (int i = 0; i < 9; i++) at0[(size_t)i].pos = make_float3((float)i, 1.0f, 2.0f), at0[(size_t)i].radius = 1.0f;
    ParseVelocities(write_file("good", "7 2.5 0 1\n8 -1 0.125 3\n"), 9, v, why);
    MoveSpheres(at0, v, 3, now);
    expect(now.size() == 9 && now[7].pos.x == 7.0f + 7.5f && now[7].pos.z == 5.0f && now[8].pos.y == 1.375f && now[0].pos.x == 0.0f,
           "the scene of frame 3");
  }
  printf("temporal_motion_sanitize: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
