// pathtrace_main.cpp -- command-line front end equivalent to the single-frame mode of
// src/main.cu:18-83,179-193, written against the look-alike headers exactly as main.cu is
// written against the reference's (Scene / Renderer / Camera / OutputBuffer).
// Same flags, defaults, banner and timing line; -i (OpenGL window) is accepted and reported as
// unsupported.  -d with --denoise-weights FILE runs the reference's CNN denoiser
// (DenoiseNet.h, pt_denoiser_*) on the frame in place after every Render() of the headless frame
// loop, as the interactive loop body does (main.cu:146-152); the saved EXR is the last denoised frame.
// (In the reference's single-frame mode -d only changes how the buffer is allocated; here the
// headless loop stands in for the interactive one, so -d denoises.)
// Additions: --rng, --max-bounces, --spheres N (seeded random scene), --frames N (headless
// stand-in for the interactive loop main.cu:146-177: N x Render() into the same device buffer),
// --poses FILE (scripted fly-through: one "x y z yaw pitch" line per frame, the pose-list format of
// collect_data.py:20-31; generator state carries over from frame to frame like the reference's
// interactive mode, per-frame times are summarised), --gpus N (the frame row-tiled over devices
// --device .. --device+N-1 by one process: MultiRenderer / pt_mgpu_*, RCCL gather to the first device), --progressive N
// (the still frame refined in N passes of -s samples each into one buffer: ProgressiveRenderer / pt_progressive_*; the
// saved frame is bit for bit the one -s N*S writes, the one-pass variant of the interactive loop with the camera at rest),
// --filter (the weights-free denoiser, FeatureFilter / pt_filter_*: every frame of the headless loop and every progressive pass
// is filtered in place after Render(), where -d would run the network; the saved EXR and bitmaps hold the filtered frame),
// --temporal (with --frames / --poses: TemporalAccumulator / pt_temporal_* accumulates every frame of the headless loop in place
// after Render() and before --filter or -d; the filter then takes the accumulator's per-pixel counts),
// --velocities FILE (with --frames / --poses: the spheres listed move at a constant velocity, the scene is uploaded before every
// frame's Render(), and --temporal accumulates through pt_temporal_run_scene, which follows them),
// --filter-spatial-below N (with --filter: the filter's spatial variance estimate, pt_filter_set_spatial, for pixels with fewer
// than N samples),
// --temporal-fast-cap X (with --temporal: the accumulator's responsive history, pt_temporal_set_antilag, against lagging light),
// --tonemap CURVE (ToneMapper / pt_tonemap_*: every frame of the headless loop and every progressive pass goes through the
// session after --temporal, --filter and -d, so that --tonemap-adapt acts as eye adaptation; the last frame's sRGB picture is
// written to <output>_tm.ppm; the frame itself, hence the EXR, the bitmaps and --preview, keeps its bytes),
// --compare REF.exr (FrameCompare / pt_compare_*: the final colour of every frame of the headless loop and of every progressive
// pass is compared on the device with the colour of REF, an EXR of the same size read by ExrReader.h, after --temporal, --filter
// and -d and before --tonemap; one "compare:" line per frame or pass),
// --materials FILE | smallpt (Material.h, pt_renderer_set_materials: a material per sphere -- mirror, glossy, glass -- for the
// single frame and the headless loop; every stage behind Render() only sees frames.  Not with --progressive, --batch or --gpus),
// --direct-light (pt_renderer_set_light_sampling: every diffuse hit also samples the emitting spheres; alone or with --materials,
// in the single frame and the headless loop, every stage behind Render() as before.  Not with --progressive, --batch or --gpus),
// --sky FILE | clear (Sky.h, pt_renderer_set_sky: a ray that leaves the scene takes a sky's radiance, and with --direct-light the
// sun is sampled like a lamp; alone or with --materials and --direct-light, in the single frame and the headless loop, every stage
// behind Render() as before.  Not with --progressive, --batch or --gpus).
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "Camera.h"
#include "DenoiseNet.h"
#include "Denoiser.h"
#include "ExrReader.h"
#include "FeatureFilter.h"
#include "FrameCompare.h"
#include "Material.h"
#include "Sky.h"
#include "MultiRenderer.h"
#include "OutputBuffer.h"
#include "ProgressiveRenderer.h"
#include "Renderer.h"
#include "Scene.h"
#include "TemporalAccumulator.h"
#include "ToneMapper.h"
#include "Velocities.h"

static void usage() {
  std::cout << "cuda-pathtrace" << std::endl
            << "Options:\n"
               "  -h [ --help ]                 Print help messages\n"
               "  -t [ --threads-per-block ] arg Number of threads per block in 2D CUDA scheduling grid. (ignored)\n"
               "  --size arg                    Size of the screen in pixels\n"
               "  -s [ --samples ] arg          Number of samples per pixel\n"
               "  --device arg                  Which device to use for rendering\n"
               "  -d [ --denoising ]            Use denoising neural network (needs --denoise-weights)\n"
               "  -i [ --interactive ]          Interactive mode (unsupported; see --frames)\n"
               "  --nobitmap                    Don't output bitmaps for each channel\n"
               "  -o [ --output ] arg           Prefix of output file/path\n"
               "  -x [ --camera-x ] arg         Starting camera position x\n"
               "  -y [ --camera-y ] arg         Starting camera position y\n"
               "  -z [ --camera-z ] arg         Starting camera position z\n"
               "  -c [ --camera-yaw ] arg       Starting camera view yaw\n"
               "  -p [ --camera-pitch ] arg     Starting camera view pitch\n"
               "  --rng arg                     xorwow (default, reference parity) | philox\n"
               "  --max-bounces arg             path length cap (default 5)\n"
               "  --spheres arg                 render a seeded random scene of N spheres\n"
               "  --frames arg                  render N frames back to back (headless interactive loop)\n"
               "  --poses arg                   fly-through: file with one 'x y z yaw pitch' line per frame\n"
               "  --batch                       with --poses: render the fly-through in batches of 32 frames per launch\n"
               "  --gpus arg                    row-tile the frame over N devices starting at --device (RCCL gather)\n"
               "  --preview arg                 also write the display-packed frame (Denoiser) as a binary PPM\n"
               "  --denoise-weights arg         with -d: PTDN weight file of the denoising network\n"
               "  --denoise-precision arg       with -d: float (default) | half (fp16 operands, fp32 accumulation)\n"
               "  --progressive arg             refine the still frame in N passes of -s samples each (one buffer)\n"
               "  --adaptive arg                with --progressive: stop pixels whose mean luminance has a relative\n"
               "                                standard error <= arg; ends early when no pixel is active\n"
               "  --adaptive-min arg            with --adaptive: no pixel stops before this many samples (default 16)\n"
               "  --adaptive-radius arg         with --adaptive: dilation radius 0..4 (default 1)\n"
               "  --filter                      denoise without weights: variance-guided a-trous filter on every frame\n"
               "  --filter-iterations arg       with --filter: a-trous iterations 1..8 (default 5)\n"
               "  --filter-sigma arg            with --filter: the four stops l,n,a,z (default 4,0.35,0.1,1)\n"
               "  --filter-spatial-below arg    with --filter: pixels with fewer than arg samples (a number >= 1, or all) estimate their\n"
               "                                variance from their neighbours on the same surface (default: off)\n"
               "  --filter-spatial-radius arg   with --filter-spatial-below: the window is (2 arg + 1)^2 pixels, 1 .. 3 (default 2)\n"
               "  --temporal                    with --frames / --poses: reproject and accumulate every frame over the last ones\n"
               "  --temporal-cap arg            with --temporal: cap of the accumulated history in samples, >= 1 (default 256)\n"
               "  --temporal-fast-cap arg       with --temporal: responsive history: keep a second history of at most arg samples\n"
               "                                (>= 1 and < the cap) and clamp the long one into its neighbourhood range, so that\n"
               "                                shadows and indirect light of moving spheres do not lag (default: off)\n"
               "  --temporal-clamp-sigma arg    with --temporal-fast-cap: half-width of the clamp box in standard deviations, > 0\n"
               "                                (default 1)\n"
               "  --temporal-clamp-radius arg   with --temporal-fast-cap: the window is (2 arg + 1)^2 pixels, 1 .. 3 (default 1)\n"
               "  --velocities arg              with --frames / --poses: file of 'index vx vy vz' lines; sphere index moves by v per frame\n"
               "                                (with --temporal every pixel follows the sphere it shows)\n"
               "  --materials arg               file of 'index kind [param]' lines (kind: diffuse | mirror | glossy rho | glass eta), or\n"
               "                                'smallpt': sphere 6 a mirror, sphere 7 glass of index 1.5; unlisted spheres are diffuse\n"
               "  --direct-light                sample the emitting spheres at every diffuse hit (next-event estimation); alone or with\n"
               "                                --materials; not with --progressive, --batch or --gpus\n"
               "  --sky arg                     file of 'zenith r g b', 'horizon r g b', 'ground r g b', 'sun dx dy dz cos r g b' lines, or\n"
               "                                'clear': a clear day; rays that leave the scene take the sky's light, and --direct-light\n"
               "                                samples the sun; not with --progressive, --batch or --gpus\n"
               "  --tonemap arg                 clamp | reinhard | aces: also write the tone-mapped picture <output>_tm.ppm\n"
               "  --exposure arg                with --tonemap: auto (default, metered on the device) or a number > 0\n"
               "  --tonemap-key arg             with --tonemap: luminance the metered mean is mapped to (default 0.18)\n"
               "  --tonemap-white arg           with --tonemap reinhard: luminance that maps to white (default 4)\n"
               "  --tonemap-adapt arg           with --tonemap: share of the way to the metered exposure per frame, (0, 1] (default 1)\n"
               "  --tonemap-encode arg          with --tonemap: srgb (default) | linear\n"
               "  --compare arg                 compare every frame or pass with the colour of this EXR: rms, psnr, relmse, ssim\n"
            << std::endl;
}

int main(int argc, const char** argv) {
  // default arguments (main.cu:20-29)
  int size = 512;
  int threadsPerBlock = 8;
  int samplesPerPixel = 4;
  int cudaDevice = 0;
  float cameraPos[3] = {50.0f, 52.0f, 295.6f};
  float cameraView[2] = {-90.0f, 0.0f};
  bool denoising = false, interactive = false, noBitmap = false;
  std::string outputName = "output/out";
  std::string rng = "xorwow";
  int maxBounces = 5, nSpheres = 0, frames = 1, gpus = 1;
  std::string posesFile, previewFile, denoiseWeights, denoisePrecision, velocitiesFile, materialsArg, skyArg;
  bool denoisePrecisionGiven = false;
  bool directLight = false;  // --direct-light: Renderer::SetLightSampling
  bool batch = false;        // --poses: all frames in one call (one launch per 32 frames)
  int progressive = 0;       // --progressive N: N passes of samplesPerPixel samples into one frame (0 = off)
  bool progressiveGiven = false, framesGiven = false, gpusGiven = false;
  // --adaptive TOL (with --progressive): adaptive sampling, pt_progressive_set_adaptive (floor: the library's Python default)
  bool adaptiveGiven = false;
  double adaptiveTol = 0.0;
  int adaptiveMin = 16, adaptiveRadius = 1;
  const float adaptiveFloor = 0.05f;
  bool adaptiveMinGiven = false, adaptiveRadiusGiven = false;
  // --filter: the feature-guided filter (pt_filter_*) in place after every Render() / progressive pass
  bool filtering = false, filterIterationsGiven = false, filterSigmaGiven = false;
  int filterIterations = 5;
  std::string filterSigma;
  // --filter-spatial-below N [--filter-spatial-radius R]: the filter's spatial variance estimate (pt_filter_set_spatial)
  bool spatialBelowGiven = false, spatialRadiusGiven = false;
  std::string spatialBelow;
  pt_filter_spatial_opts spatialOpts;
  pt_filter_spatial_opts_default(&spatialOpts);
  // --temporal: the temporal accumulator (pt_temporal_*) in place after every Render() of the frame loop
  bool temporal = false, temporalCapGiven = false;
  double temporalCap = 256.0;
  // --temporal-fast-cap [--temporal-clamp-sigma, --temporal-clamp-radius]: the responsive history (pt_temporal_set_antilag)
  bool fastCapGiven = false, clampSigmaGiven = false, clampRadiusGiven = false;
  pt_temporal_antilag_opts antilagOpts;
  pt_temporal_antilag_opts_default(&antilagOpts);
  // --tonemap CURVE: the tone-mapping session (pt_tonemap_*) after every other stage of a frame
  std::string tonemapCurve, tonemapExposure, tonemapEncode;
  bool tonemapGiven = false;
  const char* tonemapOption = NULL;  // the first --exposure / --tonemap-* option seen
  double tonemapKey = 0.18, tonemapWhite = 4.0, tonemapAdapt = 1.0;
  bool tonemapKeyGiven = false, tonemapWhiteGiven = false, tonemapAdaptGiven = false;
  // --compare REF.exr: the comparison session (pt_compare_*) after every other stage of a frame and before the tone mapper
  std::string compareFile;
  void* batch_frames = NULL;

  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto value = [&](const char* what) -> const char* {
      if (i + 1 >= argc) {
        std::cerr << "ERROR: the required argument for option '" << what << "' is missing" << std::endl << std::endl;
        usage();
        exit(1);
      }
      return argv[++i];
    };
    if (a == "-h" || a == "--help") { usage(); return 0; }
    else if (a == "-t" || a == "--threads-per-block") threadsPerBlock = atoi(value("--threads-per-block"));
    else if (a == "--size") size = atoi(value("--size"));
    else if (a == "-s" || a == "--samples") samplesPerPixel = atoi(value("--samples"));
    else if (a == "--device") cudaDevice = atoi(value("--device"));
    else if (a == "-d" || a == "--denoising") denoising = true;
    else if (a == "-i" || a == "--interactive") interactive = true;
    else if (a == "--nobitmap") noBitmap = true;
    else if (a == "-o" || a == "--output") outputName = value("--output");
    else if (a == "-x" || a == "--camera-x") cameraPos[0] = (float)atof(value("--camera-x"));
    else if (a == "-y" || a == "--camera-y") cameraPos[1] = (float)atof(value("--camera-y"));
    else if (a == "-z" || a == "--camera-z") cameraPos[2] = (float)atof(value("--camera-z"));
    else if (a == "-c" || a == "--camera-yaw") cameraView[0] = (float)atof(value("--camera-yaw"));
    else if (a == "-p" || a == "--camera-pitch") cameraView[1] = (float)atof(value("--camera-pitch"));
    else if (a == "--rng") rng = value("--rng");
    else if (a == "--max-bounces") maxBounces = atoi(value("--max-bounces"));
    else if (a == "--spheres") nSpheres = atoi(value("--spheres"));
    else if (a == "--frames") { frames = atoi(value("--frames")); framesGiven = true; }
    else if (a == "--gpus") { gpus = atoi(value("--gpus")); gpusGiven = true; }
    else if (a == "--progressive") { progressive = atoi(value("--progressive")); progressiveGiven = true; }
    else if (a == "--adaptive") { adaptiveTol = atof(value("--adaptive")); adaptiveGiven = true; }
    else if (a == "--adaptive-min") { adaptiveMin = atoi(value("--adaptive-min")); adaptiveMinGiven = true; }
    else if (a == "--adaptive-radius") { adaptiveRadius = atoi(value("--adaptive-radius")); adaptiveRadiusGiven = true; }
    else if (a == "--filter") filtering = true;
    else if (a == "--filter-iterations") { filterIterations = atoi(value("--filter-iterations")); filterIterationsGiven = true; }
    else if (a == "--filter-sigma") { filterSigma = value("--filter-sigma"); filterSigmaGiven = true; }
    else if (a == "--filter-spatial-below") { spatialBelow = value("--filter-spatial-below"); spatialBelowGiven = true; }
    else if (a == "--filter-spatial-radius") { spatialOpts.radius = atoi(value("--filter-spatial-radius")); spatialRadiusGiven = true; }
    else if (a == "--temporal") temporal = true;
    else if (a == "--temporal-cap") { temporalCap = atof(value("--temporal-cap")); temporalCapGiven = true; }
    else if (a == "--temporal-fast-cap") { antilagOpts.fast_cap = (float)atof(value("--temporal-fast-cap")); fastCapGiven = true; }
    else if (a == "--temporal-clamp-sigma") { antilagOpts.clamp_sigma = (float)atof(value("--temporal-clamp-sigma")); clampSigmaGiven = true; }
    else if (a == "--temporal-clamp-radius") { antilagOpts.clamp_radius = atoi(value("--temporal-clamp-radius")); clampRadiusGiven = true; }
    else if (a == "--tonemap") { tonemapCurve = value("--tonemap"); tonemapGiven = true; }
    else if (a == "--exposure") { tonemapExposure = value("--exposure"); if (!tonemapOption) tonemapOption = "--exposure"; }
    else if (a == "--tonemap-key") { tonemapKey = atof(value("--tonemap-key")); tonemapKeyGiven = true; if (!tonemapOption) tonemapOption = "--tonemap-key"; }
    else if (a == "--tonemap-white") { tonemapWhite = atof(value("--tonemap-white")); tonemapWhiteGiven = true; if (!tonemapOption) tonemapOption = "--tonemap-white"; }
    else if (a == "--tonemap-adapt") { tonemapAdapt = atof(value("--tonemap-adapt")); tonemapAdaptGiven = true; if (!tonemapOption) tonemapOption = "--tonemap-adapt"; }
    else if (a == "--tonemap-encode") { tonemapEncode = value("--tonemap-encode"); if (!tonemapOption) tonemapOption = "--tonemap-encode"; }
    else if (a == "--compare") compareFile = value("--compare");
    else if (a == "--poses") posesFile = value("--poses");
    else if (a == "--velocities") velocitiesFile = value("--velocities");
    else if (a == "--materials") materialsArg = value("--materials");
    else if (a == "--direct-light") directLight = true;
    else if (a == "--sky") skyArg = value("--sky");
    else if (a == "--batch") batch = true;
    else if (a == "--preview") previewFile = value("--preview");
    else if (a == "--denoise-weights") denoiseWeights = value("--denoise-weights");
    else if (a == "--denoise-precision") { denoisePrecision = value("--denoise-precision"); denoisePrecisionGiven = true; }
    else {
      std::cerr << "ERROR: unrecognised option '" << a << "'" << std::endl << std::endl;
      usage();
      return 1;
    }
  }
  int width, height;
  width = height = size;  // main.cu:66-67
  std::cout << "cuda-pathtrace 0.3" << std::endl;
  std::cout << "------------------" << std::endl;
  std::cout << "Dimensions: " << width << " x " << height << std::endl;
  std::cout << "Threads per block: " << threadsPerBlock << std::endl;
  std::cout << "Samples per pixel: " << samplesPerPixel << std::endl;
  std::cout << "Using CUDA device: " << cudaDevice << std::endl;
  const bool multi = gpus > 1 || (getenv("PT_FORCE_MGPU") && atoi(getenv("PT_FORCE_MGPU")) != 0);
  if (gpus < 1) {
    std::cerr << "ERROR: --gpus must be at least 1" << std::endl;
    return 1;
  }
  if (multi) std::cout << "Row-tiled over " << gpus << " device(s) starting at " << cudaDevice << std::endl;
  if (!interactive)
    std::cout << "Output file prefix: " << outputName << std::endl;
  else
    std::cout << "Running in interactive mode: " << (denoising ? "denoising is on" : "denoising is off") << std::endl;
  std::cout << "Camera: " << cameraPos[0] << " " << cameraPos[1] << " " << cameraPos[2] << " " << cameraView[0] << " "
            << cameraView[1] << std::endl;
  if (interactive) {
    std::cerr << "ERROR: -i needs the OpenGL window of the reference, which this build does not include; use --frames N "
                 "for a headless frame loop" << std::endl;
    return 1;
  }
  if (denoising && denoiseWeights.empty()) {
    std::cerr << "ERROR: -d needs the network's weights: --denoise-weights FILE (a PTDN file written by "
                 "cuda-pathtrace_amd/denoise_weights.py from a state_dict trained with the reference's train.py)" << std::endl;
    return 1;
  }
  if (denoisePrecisionGiven) {  // (before any device is touched)
    if (!denoising) {
      std::cerr << "ERROR: --denoise-precision needs -d: it chooses the precision of the denoising network" << std::endl;
      return 1;
    }
    if (denoisePrecision != "half" && denoisePrecision != "float") {
      std::cerr << "ERROR: --denoise-precision '" << denoisePrecision << "': half or float" << std::endl;
      return 1;
    }
  }
  if (denoising && batch) {
    std::cerr << "ERROR: -d cannot be combined with --batch: the denoiser runs after every frame of the loop" << std::endl;
    return 1;
  }
  pt_filter_opts filterOpts;
  pt_filter_opts_default(&filterOpts);
  if ((filterIterationsGiven || filterSigmaGiven) && !filtering) {  // (before any device is touched)
    std::cerr << "ERROR: " << (filterIterationsGiven ? "--filter-iterations" : "--filter-sigma")
              << " needs --filter: it sets an option of the feature-guided filter" << std::endl;
    return 1;
  }
  if (spatialBelowGiven && !filtering) {
    std::cerr << "ERROR: --filter-spatial-below needs --filter: it is the filter's variance estimate for pixels with few samples" << std::endl;
    return 1;
  }
  if (spatialRadiusGiven && !spatialBelowGiven) {
    std::cerr << "ERROR: --filter-spatial-radius needs --filter-spatial-below: it sizes the window of the variance estimate" << std::endl;
    return 1;
  }
  if (filtering) {
    if (denoising) {
      std::cerr << "ERROR: --filter cannot be combined with -d: choose the filter or the network" << std::endl;
      return 1;
    }
    if (batch) {
      std::cerr << "ERROR: --filter cannot be combined with --batch: the filter runs after every frame of the loop" << std::endl;
      return 1;
    }
    if (filterIterationsGiven && (filterIterations < 1 || filterIterations > 8)) {
      std::cerr << "ERROR: --filter-iterations " << filterIterations << ": 1 .. 8" << std::endl;
      return 1;
    }
    filterOpts.iterations = filterIterations;
    if (filterSigmaGiven) {
      float v[4];
      char extra;
      const int got = sscanf(filterSigma.c_str(), "%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &extra);
      bool ok = got == 4;
      for (int k = 0; ok && k < 4; k++) ok = v[k] > 0.0f && v[k] <= 3.4028234663852886e38f;
      if (!ok) {
        std::cerr << "ERROR: --filter-sigma '" << filterSigma << "': four finite numbers > 0 as l,n,a,z (luminance, normal, albedo, depth)"
                  << std::endl;
        return 1;
      }
      filterOpts.sigma_l = v[0], filterOpts.sigma_n = v[1], filterOpts.sigma_a = v[2], filterOpts.sigma_z = v[3];
    }
    if (spatialBelowGiven) {  // the library's own host checks, before any device is touched
      if (spatialBelow == "all") {
        spatialOpts.below = PT_FILTER_SPATIAL_ALL;
      } else {
        char* end = NULL;
        const unsigned long long v = strtoull(spatialBelow.c_str(), &end, 10);
        const bool digits = !spatialBelow.empty() && spatialBelow.find_first_not_of("0123456789") == std::string::npos;
        if (!digits || *end != '\0' || v < 1 || v > 0xFFFFFFFFull) {
          std::cerr << "ERROR: --filter-spatial-below '" << spatialBelow << "': a sample count 1 .. 4294967295, or all (leave the option out for off)"
                    << std::endl;
          return 1;
        }
        spatialOpts.below = (unsigned int)v;
      }
      if (pt_filter_spatial_check(&spatialOpts) != PT_OK) {
        std::cerr << "ERROR: --filter-spatial-radius: " << pt_last_error() << std::endl;
        return 1;
      }
    }
  }
  pt_temporal_opts temporalOpts;
  pt_temporal_opts_default(&temporalOpts);
  if (temporalCapGiven && !temporal) {  // (before any device is touched)
    std::cerr << "ERROR: --temporal-cap needs --temporal: it caps the accumulator's history" << std::endl;
    return 1;
  }
  if (fastCapGiven && !temporal) {
    std::cerr << "ERROR: --temporal-fast-cap needs --temporal: it is the accumulator's second, short history" << std::endl;
    return 1;
  }
  if ((clampSigmaGiven || clampRadiusGiven) && !fastCapGiven) {
    std::cerr << "ERROR: " << (clampSigmaGiven ? "--temporal-clamp-sigma" : "--temporal-clamp-radius")
              << " needs --temporal-fast-cap: it shapes the clamp of the responsive history" << std::endl;
    return 1;
  }
  if (temporal) {
    if (progressiveGiven) {
      std::cerr << "ERROR: --temporal cannot be combined with --progressive: a still frame has the progressive session" << std::endl;
      return 1;
    }
    if (batch) {
      std::cerr << "ERROR: --temporal cannot be combined with --batch: the accumulator runs after every frame of the loop" << std::endl;
      return 1;
    }
    if (!framesGiven && posesFile.empty()) {
      std::cerr << "ERROR: --temporal needs --frames or --poses: it accumulates the frames of the headless loop" << std::endl;
      return 1;
    }
    if (temporalCapGiven && (!(temporalCap >= 1.0) || !(temporalCap <= 3.4028234663852886e38))) {
      std::cerr << "ERROR: --temporal-cap " << temporalCap << ": a finite number of samples >= 1" << std::endl;
      return 1;
    }
    temporalOpts.history_cap = (float)temporalCap;
    if (fastCapGiven) {  // the library's own host checks, before any device is touched
      if (!(antilagOpts.fast_cap >= 1.0f)) {
        std::cerr << "ERROR: --temporal-fast-cap: fast_cap " << antilagOpts.fast_cap << " must be >= 1 (leave the option out for off)" << std::endl;
        return 1;
      }
      if (pt_temporal_antilag_check(&antilagOpts, temporalOpts.history_cap) != PT_OK) {
        std::cerr << "ERROR: --temporal-fast-cap: " << pt_last_error() << std::endl;
        return 1;
      }
    }
  }
  // --velocities: the list and the scene of frame 0 on the host (before any device is touched)
  std::vector<SphereVelocity> velocities;
  std::vector<Sphere> spheresAt0, spheresNow;
  if (!velocitiesFile.empty()) {
    if (batch || progressiveGiven) {
      std::cerr << "ERROR: --velocities cannot be combined with " << (batch ? "--batch" : "--progressive")
                << ": the scene is uploaded before every frame of the loop" << std::endl;
      return 1;
    }
    if (!framesGiven && posesFile.empty()) {
      std::cerr << "ERROR: --velocities needs --frames or --poses: the spheres move from frame to frame of the headless loop" << std::endl;
      return 1;
    }
    const int count = nSpheres > 0 ? nSpheres : 9;
    std::string why;
    if (!ParseVelocities(velocitiesFile, count, velocities, why)) {
      std::cerr << "ERROR: --velocities: " << why << std::endl;
      return 1;
    }
    spheresAt0.resize((size_t)count);
    pt_sphere* host = reinterpret_cast<pt_sphere*>(spheresAt0.data());
    if ((nSpheres > 0 ? pt_scene_random(nSpheres, 1, 1, host) : pt_scene_cornell(host)) != PT_OK) {
      std::cerr << "ERROR: --velocities: " << pt_last_error() << std::endl;
      return 1;
    }
  }
  // --materials: the table on the host, checked by the library's own host checks (before any device is touched)
  std::vector<pt_material> materials;
  if (!materialsArg.empty()) {
    const char* other = progressiveGiven ? "--progressive" : batch ? "--batch" : multi ? "--gpus" : NULL;
    if (other) {
      std::cerr << "ERROR: --materials cannot be combined with " << other
                << ": the materials kernel renders single frames on one device (no progressive passes, no frame batches)" << std::endl;
      return 1;
    }
    const int count = nSpheres > 0 ? nSpheres : 9;
    std::string why;
    if (!(materialsArg == "smallpt" ? SmallptMaterials(count, materials, why) : ParseMaterials(materialsArg, count, materials, why))) {
      std::cerr << "ERROR: --materials: " << why << std::endl;
      return 1;
    }
  }
  if (directLight) {  // (before any device is touched)
    const char* other = progressiveGiven ? "--progressive" : batch ? "--batch" : multi ? "--gpus" : NULL;
    if (other) {
      std::cerr << "ERROR: --direct-light cannot be combined with " << other
                << ": the light-sampling kernel renders single frames on one device (no progressive passes, no frame batches)" << std::endl;
      return 1;
    }
  }
  // --sky: the description on the host, checked by the library's own host checks (before any device is touched)
  Sky sky = ClearSky();
  if (!skyArg.empty()) {
    const char* other = progressiveGiven ? "--progressive" : batch ? "--batch" : multi ? "--gpus" : NULL;
    if (other) {
      std::cerr << "ERROR: --sky cannot be combined with " << other
                << ": the sky kernel renders single frames on one device (no progressive passes, no frame batches)" << std::endl;
      return 1;
    }
    std::string why;
    if (skyArg != "clear" && !ParseSky(skyArg, sky, why)) {
      std::cerr << "ERROR: --sky: " << why << std::endl;
      return 1;
    }
  }
  pt_tonemap_opts tonemapOpts;
  pt_tonemap_opts_default(&tonemapOpts);
  if (tonemapOption && !tonemapGiven) {  // (before any device is touched)
    std::cerr << "ERROR: " << tonemapOption << " needs --tonemap: it sets an option of the tone mapper" << std::endl;
    return 1;
  }
  if (tonemapGiven) {
    if (batch) {
      std::cerr << "ERROR: --tonemap cannot be combined with --batch: the tone mapper runs after every frame of the loop" << std::endl;
      return 1;
    }
    if (tonemapCurve == "clamp") tonemapOpts.curve = PT_TONEMAP_CLAMP;
    else if (tonemapCurve == "reinhard") tonemapOpts.curve = PT_TONEMAP_REINHARD;
    else if (tonemapCurve == "aces") tonemapOpts.curve = PT_TONEMAP_ACES;
    else {
      std::cerr << "ERROR: --tonemap '" << tonemapCurve << "': clamp, reinhard or aces" << std::endl;
      return 1;
    }
    if (!tonemapEncode.empty()) {
      if (tonemapEncode == "srgb") tonemapOpts.encode = PT_ENCODE_SRGB;
      else if (tonemapEncode == "linear") tonemapOpts.encode = PT_ENCODE_LINEAR;
      else {
        std::cerr << "ERROR: --tonemap-encode '" << tonemapEncode << "': srgb or linear" << std::endl;
        return 1;
      }
    }
    if (!tonemapExposure.empty() && tonemapExposure != "auto") {
      char* end = NULL;
      const double e = strtod(tonemapExposure.c_str(), &end);
      if (end == tonemapExposure.c_str() || *end != '\0' || !(e > 0.0) || !(e <= 3.4028234663852886e38) || (float)e == 0.0f) {
        std::cerr << "ERROR: --exposure '" << tonemapExposure << "': auto or a finite number > 0" << std::endl;
        return 1;
      }
      tonemapOpts.exposure = (float)e;
    }
    if (tonemapKeyGiven && (!(tonemapKey > 0.0) || !(tonemapKey <= 3.4028234663852886e38) || (float)tonemapKey == 0.0f)) {
      std::cerr << "ERROR: --tonemap-key " << tonemapKey << ": a finite luminance > 0" << std::endl;
      return 1;
    }
    if (tonemapWhiteGiven && !(tonemapWhite >= 1e-18 && tonemapWhite <= 1e18)) {
      std::cerr << "ERROR: --tonemap-white " << tonemapWhite << ": a luminance in 1e-18 .. 1e18" << std::endl;
      return 1;
    }
    if (tonemapAdaptGiven && !(tonemapAdapt > 0.0 && tonemapAdapt <= 1.0 && (float)tonemapAdapt > 0.0f)) {
      std::cerr << "ERROR: --tonemap-adapt " << tonemapAdapt << ": a rate in (0, 1]" << std::endl;
      return 1;
    }
    tonemapOpts.key = (float)tonemapKey, tonemapOpts.white = (float)tonemapWhite, tonemapOpts.adapt = (float)tonemapAdapt;
  }
  ptexr::FeatureImage compareReference;
  if (!compareFile.empty()) {  // (before any device is touched, and before anything is rendered)
    if (batch) {
      std::cerr << "ERROR: --compare cannot be combined with --batch: the comparison runs after every frame of the loop" << std::endl;
      return 1;
    }
    std::string why;
    if (!ptexr::LoadFeatureEXR(compareFile, &compareReference, &why)) {
      std::cerr << "ERROR: --compare " << compareFile << ": " << why << std::endl;
      return 1;
    }
    if (compareReference.width != width || compareReference.height != height) {
      std::cerr << "ERROR: --compare " << compareFile << ": the reference is " << compareReference.width << " x " << compareReference.height
                << ", the frame " << width << " x " << height << std::endl;
      return 1;
    }
  }
  if ((adaptiveGiven || adaptiveMinGiven || adaptiveRadiusGiven) && !progressiveGiven) {  // (before any device is touched)
    std::cerr << "ERROR: " << (adaptiveGiven ? "--adaptive" : adaptiveMinGiven ? "--adaptive-min" : "--adaptive-radius")
              << " needs --progressive: adaptive sampling refines a progressive session" << std::endl;
    return 1;
  }
  if ((adaptiveMinGiven || adaptiveRadiusGiven) && !adaptiveGiven) {
    std::cerr << "ERROR: " << (adaptiveMinGiven ? "--adaptive-min" : "--adaptive-radius") << " needs --adaptive" << std::endl;
    return 1;
  }
  if (adaptiveGiven) {
    if (!(adaptiveTol >= 0.0) || !(adaptiveTol <= 3.4e38)) {
      std::cerr << "ERROR: --adaptive " << adaptiveTol << ": the tolerance must be a finite number >= 0" << std::endl;
      return 1;
    }
    if (adaptiveMin < 2) {
      std::cerr << "ERROR: --adaptive-min " << adaptiveMin << ": at least 2 samples (the variance needs two)" << std::endl;
      return 1;
    }
    if (adaptiveRadius < 0 || adaptiveRadius > 4) {
      std::cerr << "ERROR: --adaptive-radius " << adaptiveRadius << ": 0 .. 4" << std::endl;
      return 1;
    }
  }
  if (progressiveGiven) {  // (before any device is touched, like the weight check below)
    const char* other = framesGiven ? "--frames" : !posesFile.empty() ? "--poses" : batch ? "--batch" : gpusGiven ? "--gpus" : NULL;
    if (other) {
      std::cerr << "ERROR: --progressive cannot be combined with " << other << ": a progressive session refines one still frame on one device"
                << std::endl;
      return 1;
    }
    if (progressive < 1) {
      std::cerr << "ERROR: --progressive needs at least one pass (got " << progressive << ")" << std::endl;
      return 1;
    }
    const long long total = (long long)progressive * samplesPerPixel;
    if (samplesPerPixel < 1 || total < 2 || total > INT_MAX) {
      std::cerr << "ERROR: --progressive " << progressive << " with -s " << samplesPerPixel << " makes " << total
                << " samples per pixel; a session needs 2 .. " << INT_MAX << " (one sample is the reference's unjittered frame: use -s 1)"
                << std::endl;
      return 1;
    }
  }
  if (denoising) {  // the weight file is checked before any device is touched (host only)
    std::ifstream wf(denoiseWeights.c_str(), std::ios::binary);
    std::vector<char> blob((std::istreambuf_iterator<char>(wf)), std::istreambuf_iterator<char>());
    if (!wf.good() && !wf.eof()) blob.clear();
    if (blob.empty() || pt_denoiser_weights_check(blob.data(), blob.size()) != PT_OK) {
      std::cerr << "ERROR: --denoise-weights " << denoiseWeights << ": "
                << (blob.empty() ? "cannot read the file" : pt_last_error()) << std::endl;
      return 1;
    }
  }

  // set device (main.cu:86)
  gpuErrchk(pt_set_device(cudaDevice));

  // load scene and create renderer (main.cu:125-128)
  Scene scene = nSpheres > 0 ? Scene::Random(nSpheres, 1, true) : Scene();
  pt_renderer_opts opts;
  pt_renderer_opts_default(&opts);
  opts.max_bounces = maxBounces;
  opts.rng_mode = rng == "philox" ? PT_RNG_PHILOX : PT_RNG_XORWOW;
  // one device: the reference's Renderer; several: the same interface over pt_mgpu_* (frame and scene stay on
  // the first device, where main.cu has them)
  Renderer* single = NULL;
  MultiRenderer* tiled = NULL;
  if (multi) {
    std::vector<int> devices;
    for (int g = 0; g < gpus; g++) devices.push_back(cudaDevice + g);
    tiled = new MultiRenderer(devices, width, height, samplesPerPixel, threadsPerBlock, &opts);
    std::cout << "Exchange: " << tiled->Backend() << std::endl;
  } else {
    single = new Renderer(width, height, samplesPerPixel, threadsPerBlock, opts);
    if (!materials.empty()) single->SetMaterials(materials);
    if (directLight) single->SetLightSampling(true);
    if (!skyArg.empty()) single->SetSky(&sky);
  }
  // -d: the network for this frame size on the first device (after a multi-GPU frame's gather the frame lives there)
  DenoiseNet* net =
      denoising ? new DenoiseNet(width, height, denoiseWeights, 1, denoisePrecision == "half" ? PT_DENOISE_F16 : PT_DENOISE_F32) : NULL;
  // --filter: likewise on the first device, after the gather
  FeatureFilter* filter = filtering ? new FeatureFilter(width, height, filterOpts) : NULL;
  if (filter && spatialBelowGiven) filter->SetSpatial(spatialOpts.below, spatialOpts.radius);
  // --temporal: likewise; with --filter its per-pixel counts replace the filter's uniform count
  TemporalAccumulator* accumulator = temporal ? new TemporalAccumulator(width, height, temporalOpts) : NULL;
  if (accumulator && fastCapGiven) accumulator->SetAntilag(antilagOpts.fast_cap, antilagOpts.clamp_sigma, antilagOpts.clamp_radius);
  unsigned int* d_temporalCounts = NULL;
  if (accumulator && filter) gpuErrchk(pt_malloc((void**)&d_temporalCounts, (size_t)width * height * sizeof(unsigned int)));
  // --tonemap: likewise; it reads the frame the other stages left and writes its own RGBA8 image
  ToneMapper* mapper = tonemapGiven ? new ToneMapper(width, height, tonemapOpts) : NULL;
  // --compare: likewise; it reads the frame the other stages left, before the tone mapper, and writes nothing
  FrameCompare* comparison = compareFile.empty() ? NULL : new FrameCompare(width, height, compareReference.buffer.data());
  float denoiseTime = 0.0f, filterTime = 0.0f, temporalTime = 0.0f, tonemapTime = 0.0f, compareTime = 0.0f;
  auto compare = [&](const OutputBuffer& b) {
    compareTime = comparison->Compare(b);
    const pt_compare_values v = comparison->Result();
    char text[256];
    snprintf(text, sizeof(text), "compare: rms %.17g psnr %.17g relmse %.17g ssim %.17g (saturated %llu, nonfinite %llu)", v.rms, v.psnr,
             v.relmse, v.ssim, (unsigned long long)v.saturated, (unsigned long long)v.nonfinite);
    std::cout << text << std::endl;
  };
  int frameIndex = 0;  // (of the headless loop: --velocities)
  auto render = [&](OutputBuffer b, Scene& s, const Camera& c) {
    if (!velocities.empty()) {  // the scene of this frame, uploaded before Render()
      MoveSpheres(spheresAt0, velocities, frameIndex++, spheresNow);
      s.Update(spheresNow);
    }
    const float ms = tiled ? tiled->Render(b, s, c) : single->Render(b, s, c);
    if (accumulator && !velocities.empty()) temporalTime = accumulator->Accumulate(b, samplesPerPixel, c, spheresNow, d_temporalCounts);
    else if (accumulator) temporalTime = accumulator->Accumulate(b, samplesPerPixel, c, d_temporalCounts);
    if (net) denoiseTime = net->Denoise(b);  // main.cu:148-152: Render, then the network in place
    if (filter) filterTime = filter->Filter(b, samplesPerPixel, d_temporalCounts);
    if (comparison) compare(b);
    if (mapper) tonemapTime = mapper->Map(b);
    return ms;
  };
  Camera camera(glm::vec3(cameraPos[0], cameraPos[1], cameraPos[2]), cameraView[0], cameraView[1]);  // main.cu:128 verbatim

  // allocate output buffer (main.cu:131-139)
  OutputBuffer d_buffer(width, height);
  d_buffer.AllocateGPU();

  // render frame(s) (main.cu:182-183; --frames repeats the loop body of main.cu:146-148)
  float renderTime = 0.0f;
  if (!posesFile.empty()) {
    // headless version of the interactive loop: the camera moves, the same device buffer and the
    // same renderer (generator state included) are reused every frame (main.cu:146-148)
    std::ifstream in(posesFile.c_str());
    if (!in) {
      std::cerr << "ERROR: cannot open pose file " << posesFile << std::endl;
      return 1;
    }
    std::vector<float> times;
    std::vector<Camera> cameras;
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      float x, y, z, yaw, pitch;
      if (!(ls >> x >> y >> z >> yaw >> pitch)) continue;
      cameras.push_back(Camera(glm::vec3(x, y, z), yaw, pitch));
    }
    if (cameras.empty()) {
      std::cerr << "ERROR: no poses in " << posesFile << std::endl;
      return 1;
    }
    if (batch && single) {
      // every pose is known before the first frame: one call, one launch per 32 frames (Renderer::RenderFrames); each frame
      // has its own buffer, the last one is what gets saved
      void* d_frames = NULL;
      const size_t frame_floats = (size_t)width * height * 14;
      gpuErrchk(pt_malloc(&d_frames, cameras.size() * frame_floats * sizeof(float)));
      const float ms = single->RenderFrames(static_cast<float*>(d_frames), scene, cameras);
      std::cout << "Fly-through in batches: " << cameras.size() << " frames, " << ms / cameras.size() << "ms per frame ("
                << 1000.0 * cameras.size() / ms << " fps)" << std::endl;
      d_buffer.FreeGPU();
      batch_frames = d_frames;
      d_buffer.buffer = static_cast<float*>(d_frames) + (cameras.size() - 1) * frame_floats;
      renderTime = ms / cameras.size();
      times.push_back(renderTime);
    } else {
      for (size_t f = 0; f < cameras.size(); f++) {
        renderTime = render(d_buffer, scene, cameras[f]);
        times.push_back(renderTime);
      }
    }
    std::vector<float> sorted(times);
    std::sort(sorted.begin(), sorted.end());
    double sum = 0;
    for (float t : times) sum += t;
    std::cout << "Fly-through: " << times.size() << " frames, mean " << sum / times.size() << "ms, median "
              << sorted[sorted.size() / 2] << "ms, min " << sorted.front() << "ms, max " << sorted.back() << "ms ("
              << 1000.0 * times.size() / sum << " fps)" << std::endl;
  } else if (progressiveGiven) {
    // the interactive loop with the camera at rest, refining instead of re-rendering: pass k adds samplesPerPixel samples and
    // leaves the frame of all k * samplesPerPixel in the buffer (-d: the network runs on it after every pass)
    // (--adaptive: only the pixels that have not converged; the loop ends early when none is left)
    ProgressiveRenderer session(*single, width, height);
    if (adaptiveGiven) session.SetAdaptive((float)adaptiveTol, adaptiveFloor, adaptiveMin, adaptiveRadius);
    std::vector<float> times;
    unsigned int* d_counts = NULL;
    if (adaptiveGiven) gpuErrchk(pt_malloc((void**)&d_counts, (size_t)width * height * sizeof(unsigned int)));
    std::vector<unsigned int> counts(adaptiveGiven ? (size_t)width * height : 0);
    for (int k = 0; k < progressive; k++) {
      long long active = (long long)width * height;
      if (adaptiveGiven && k > 0) {
        active = session.Active();
        if (active == 0) break;
      }
      times.push_back(session.Refine(d_buffer, scene, camera, samplesPerPixel));
      if (net) denoiseTime = net->Denoise(d_buffer);
      if (adaptiveGiven) session.Counts(d_counts);
      // --filter: with the session's count so far; under --adaptive with every pixel's own count
      if (filter) filterTime = filter->Filter(d_buffer, (int)session.Samples(), d_counts);
      if (comparison) compare(d_buffer);
      if (mapper) tonemapTime = mapper->Map(d_buffer);
      if (adaptiveGiven) {
        gpuErrchk(pt_memcpy_d2h(counts.data(), d_counts, counts.size() * sizeof(unsigned int)));
        double spp = 0;
        for (unsigned int c : counts) spp += c;
        std::cout << "Pass " << k + 1 << ": active " << 100.0 * active / ((double)width * height) << "%, mean "
                  << spp / counts.size() << " spp, " << times.back() << "ms" << std::endl;
      }
    }
    if (d_counts) gpuErrchk(pt_free(d_counts));
    std::vector<float> sorted(times);
    std::sort(sorted.begin(), sorted.end());
    double sum = 0;
    for (float t : times) sum += t;
    std::cout << "Progressive: " << times.size() << " passes of " << samplesPerPixel << " spp (" << session.Samples()
              << " spp), pass mean " << sum / times.size() << "ms, median " << sorted[sorted.size() / 2] << "ms, min "
              << sorted.front() << "ms, max " << sorted.back() << "ms" << std::endl;
    renderTime = (float)sum;
  } else {
    for (int f = 0; f < frames; f++) renderTime = render(d_buffer, scene, camera);
  }
  std::cout << "Render completed in " << renderTime << "ms (" << 1000.0f / renderTime << " fps)" << std::endl;
  if (accumulator) std::cout << "Temporal accumulation completed in " << temporalTime << "ms" << std::endl;
  if (net) std::cout << "Denoise completed in " << denoiseTime << "ms" << std::endl;
  if (filter) std::cout << "Filter completed in " << filterTime << "ms" << std::endl;
  if (comparison) std::cout << "Comparison completed in " << compareTime << "ms" << std::endl;
  if (mapper) std::cout << "Tone mapping completed in " << tonemapTime << "ms (exposure " << mapper->Exposure() << ")" << std::endl;
  if (tiled) {
    std::cout << "Tile kernel times:";
    for (int g = 0; g < gpus; g++) std::cout << " " << tiled->TileKernelMs(g) << "ms";
    std::cout << std::endl;
  }
  std::cout << std::endl;
  if (!previewFile.empty()) {
    // what the interactive mode would put on screen (main.cu:175-176): Denoiser packs the colour
    // channels to RGBA8 point sprites; here they are unpacked into a PPM instead of drawn with GL
    Denoiser denoiser(width, height, threadsPerBlock);
    void* d_vertices = NULL;
    gpuErrchk(pt_malloc(&d_vertices, (size_t)width * height * 3 * sizeof(float)));
    denoiser.Denoise(d_buffer, static_cast<float*>(d_vertices));
    std::vector<float> vertices((size_t)width * height * 3);
    gpuErrchk(pt_memcpy_d2h(vertices.data(), d_vertices, vertices.size() * sizeof(float)));
    gpuErrchk(pt_free(d_vertices));
    FILE* f = fopen(previewFile.c_str(), "wb");
    if (!f) {
      std::cerr << "ERROR: cannot write " << previewFile << std::endl;
      return 1;
    }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (size_t i = 0; i < (size_t)width * height; i++) {
      unsigned char rgba[4];
      memcpy(rgba, &vertices[3 * i + 2], 4);
      fwrite(rgba, 1, 3, f);
    }
    fclose(f);
  }
  if (mapper && !mapper->SavePPM(outputName + "_tm.ppm")) {
    std::cerr << "ERROR: cannot write " << outputName << "_tm.ppm" << std::endl;
    return 1;
  }
  // save results (main.cu:186-192)
  OutputBuffer buffer(width, height);
  buffer.AllocateCPU();
  buffer.CopyFromGPU(d_buffer);
  buffer.SaveEXR(outputName + ".exr");
  if (!noBitmap) buffer.SaveBitmaps(outputName);
  buffer.FreeCPU();
  delete net;
  delete filter;
  delete accumulator;
  delete comparison;
  delete mapper;
  if (d_temporalCounts) (void)pt_free(d_temporalCounts);
  delete single;
  delete tiled;
  if (batch_frames) (void)pt_free(batch_frames);  // (d_buffer points into it)
  else d_buffer.FreeGPU();
  scene.Free();
  return 0;
}
