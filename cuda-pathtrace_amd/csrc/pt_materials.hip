// pt_materials.hip -- per-sphere materials (pt_renderer_set_materials): DIFFUSE, MIRROR, GLOSSY and GLASS in one exact kernel.
//
// EXACT code like the pixel kernels and pt_temporal.hip: contraction off, every operation rounded once, IEEE divisions and
// square roots, in the order EXACTNESS.md A.22 fixes; tests/materials_model.py is the same definition in NumPy float32 and the
// kernel equals it bit for bit.  With an all-diffuse table the frame is the oracle's (the anchor: every line a diffuse bounce
// executes is one of trace_ray's, pt_trace.h).
//
// The family stands OUTSIDE the variant table (kVariants, pt_kernel.hip) and the launch census: it has no row, its launches do
// not go through PT_LAUNCHED, pt_debug_kernel_builds does not list it.  pt_renderer_kernel_info reports PT_VARIANT_MATERIALS.
//
// Nearest hit: tracer level 6 WITHOUT its three origin-dependent shortcuts (intersect_scene<6, PRIMARY = false, LAST = false,
// WALLS = false>, pt_intersect.h).  What is left rests on A.1, A.2 and A.8 alone -- the screen ranks the contract's own floats
// and every doubtful lane runs the literal loop -- and none of those arguments looks at where a ray starts.  The shortcuts that
// do (the staged eye terms and pixel footprints of primary rays, A.7; the wall certificate, which assumes an origin inside the
// box; the uniform grid's admission radius, A.6) are not instantiated: a refracted ray starts 0.05 INSIDE a sphere.
//
// Divergence: the four kinds meet inside a wave64.  The pieces are computed once and selected -- the cosine direction serves
// DIFFUSE and GLOSSY, the mirror direction MIRROR, GLOSSY and both reflecting arms of GLASS -- under two wave-uniform skips
// (no lane of the wave on a non-diffuse sphere; no lane on glass), so a wave that sees only diffuse surfaces runs trace_ray's
// instructions and nothing else.
//
// LIGHTS (pt_renderer_set_light_sampling, PT_VARIANT_MATERIALS_LIGHTS; EXACTNESS.md A.23, tests/lights_model.py): the second template
// parameter adds direct light sampling, everything of it under `if constexpr (LIGHTS)` -- with LIGHTS = false the instruction stream
// is the family's as it was.  Per DIFFUSE hit but the last bounce's and per emitting sphere: one direction inside the cone the
// sphere subtends, one shadow ray by the same search, and a 64-bit set per path of the lights so accounted for, whose emission the
// next hit leaves out.  The loop over lights is scalar (the list is one ballot over the staged spheres); the shadow search runs
// with every lane of the bounce loop in step, a lane without a sample following its own next ray with its result dropped, and is
// skipped when no lane of the wave has a sample.  The shadow ray is unbounded: "the nearest hit is sphere s" is what the search
// returns.  122 / 127 VGPRs, no scratch: the family's launch bound holds (profiles/lights/README.md).
//
// SKY (pt_renderer_set_sky, PT_VARIANT_MATERIALS_SKY / PT_VARIANT_MATERIALS_LIGHTS_SKY; EXACTNESS.md A.24, tests/sky_model.py): the
// third template parameter gives an escaping path the radiance of a sky -- a gradient over u.y, a ground colour, a sun disc --
// everything of it under `if constexpr (SKY)`, and a build without it keeps its arguments and its instruction stream
// (tools/sky_asm_diff.py).  The sky's constants are a kernel argument by value: wave-uniform, in scalar registers.  With LIGHTS the
// sun is the last light of the list: light_sample's sequence from the polar angle on (cone_polar, cone_direction) around a
// direction and a frame the host formed, one shadow ray with the wave converged, lit iff the search finds nothing, and a flag per
// path that keeps the next escape from counting the disc again.  118 / 119 / 122 / 127 VGPRs, no scratch (profiles/sky/README.md).
#include <cstring>

#include "pt_intersect.h"
#include "pt_internal.h"

#pragma clang fp contract(off)

namespace pt {
namespace materials {

// one row of the device table: what pt_renderer_set_materials forms on the host from a pt_material, in float32
struct Row {
  int32_t kind;  // PT_MATERIAL_*
  float param;   // GLOSSY: rho; GLASS: eta
  float inv;     // GLASS: 1.0f / eta
  float r0;      // GLASS: ((eta - 1)(eta - 1)) / ((eta + 1)(eta + 1))
};
static_assert(sizeof(Row) == sizeof(float4), "one LDS slot per sphere");

struct Step {
  F3 normal;  // nl: the first-hit feature
  F3 o, d;    // next ray
  float w;    // factor on the mask after the colour (1 where the definition has none: x * 1.0f is x)
};

// everything of a bounce after the search and the draws (EXACTNESS.md A.22).  FAST: the cheap sequences of the level-6 tracer
// (A.3: identical bits inside their verified domains; outside, `bad` is raised and the caller redoes the step with FAST = false)
template <bool FAST>
__device__ __forceinline__ Step bounce_step(F3 o, F3 d, float t, F3 centre, float u_az, float u_el, const Row m, bool& bad,
                                            const float* unit_tab, uint32_t absmask) {
  Step out;
  // today's lines (bounce_geometry, pt_device.h): pos, nl, o' = pos + nl * 0.05f, the cosine-weighted direction
  bool bad_d = false;
  const BounceGeom bg = bounce_geometry<FAST, FAST>(o, d, t, centre, u_az, u_el, bad_d, unit_tab, absmask);
  bad = bad | bad_d;
  out.normal = bg.normal;
  out.o = bg.o;
  out.d = bg.d;
  out.w = 1.0f;
  const int kind = m.kind;
  if (__builtin_amdgcn_ballot_w64(kind != PT_MATERIAL_DIFFUSE) == 0ull) return out;  // wave-uniform

  // the same pos and geometric normal again (the same operations on the same operands: the compiler keeps one copy)
  bool bad_m = false;
  const F3 pos = o + d * t;
  F3 nr = pos - centre;
  if constexpr (FAST) nr = normalize_nb(nr, bad_m); else nr = normalize(nr);
  const bool front = dot(nr, d) < 0.0f;
  const F3 nl = bg.normal;  // front ? nr : nr * -1.0f
  auto unit = [&](F3 v, bool& flag) { if constexpr (FAST) return normalize_nb(v, flag); else return normalize(v); };
  const F3 du = unit(d, bad_m);  // a primary ray is not of unit length
  const float ddn = dot(nl, du);
  const F3 mir = unit(du - nl * (2.0f * ddn), bad_m);
  const F3 gl = unit(mir + (bg.d - mir) * m.param, bad_m);  // GLOSSY: no pdf weight (the diffuse bounce has none either)
  F3 dn = kind == PT_MATERIAL_GLOSSY ? gl : mir;
  F3 on = bg.o;
  float w = 1.0f;
  if (__builtin_amdgcn_ballot_w64(kind == PT_MATERIAL_GLASS) != 0ull) {  // wave-uniform
    bool bad_g = false;
    const float nnt = front ? m.inv : m.param;
    const float k = 1.0f - (nnt * nnt) * (1.0f - ddn * ddn);
    const bool tir = !(k >= 0.0f);  // total internal reflection, and what a NaN takes: the MIRROR step, no weight
    float s;
    if constexpr (FAST) s = sqrt_cr_f32_nb(k, bad_g); else s = sqrtf(k);
    const F3 td = unit(du * nnt - nl * (ddn * nnt + s), bad_g);
    const float cx = front ? -ddn : dot(td, nr);
    const float c1 = 1.0f - cx;
    const float c5 = ((c1 * c1) * (c1 * c1)) * c1;
    const float re = m.r0 + (1.0f - m.r0) * c5;
    const float p = 0.25f + 0.5f * re;
    const bool reflect = u_az < p;
    const float wr = re / p, wt = (1.0f - re) / (1.0f - p);
    const bool glass = kind == PT_MATERIAL_GLASS;
    const bool through = glass & !tir & !reflect;
    if (glass & !tir) w = reflect ? wr : wt;
    const F3 oi = pos - nl * 0.05f;  // pushed through the surface
    if (through) {
      dn = td;
      on = oi;
    }
    bad_m = bad_m | (glass & !tir & bad_g);
  }
  if (kind != PT_MATERIAL_DIFFUSE) {
    out.o = on;
    out.d = dn;
    out.w = w;
    bad = bad | bad_m;
  }
  return out;
}

// ---- direct light sampling (EXACTNESS.md A.23; tests/lights_model.py is the same definition) -------------------------------------
// the two draws of light j at bounce n, after the bounce's own
template <int RNG>
__device__ __forceinline__ void light_draws(Rng<RNG>& rng, int n, int j, uint4& blk, float& u0, float& u1) {
  if constexpr (RNG == PT_RNG_XORWOW) {
    u0 = uniform_from_u32(xorwow_next(rng.st));
    u1 = uniform_from_u32(xorwow_next(rng.st));
  } else {
    // counter (pixel, sample, n, 1 + (j >> 1)): the path's own blocks all have word 3 = 0
    if ((j & 1) == 0) blk = philox4x32_10(make_uint4(rng.pix, rng.sample, (uint32_t)n, 1u + ((uint32_t)j >> 1)), rng.k0, rng.k1);
    u0 = uniform_from_u32((j & 1) ? blk.z : blk.x);
    u1 = uniform_from_u32((j & 1) ? blk.w : blk.y);
  }
}

struct LightSample {
  F3 l;          // direction of the shadow ray
  float cosl;    // dot(l, nl)
  float factor;  // cosl * (2 * vers) = cosl * Omega / pi
  bool outside;  // d2 > r2: the point is outside the light (false also for a NaN)
};

// the tail of a cone sample, shared by the sphere lights (A.23) and the sun (A.24): the polar angle's cosine and sine from u1 and
// vers = 1 - cos(a_max) ...
template <bool FAST>
__device__ __forceinline__ void cone_polar(float u1, float vers, float& cos_a, float& sin_a, bool& bad) {
  const float h = u1 * vers;
  cos_a = 1.0f - h;
  if constexpr (FAST) sin_a = sqrt_cr_f32_nb(h * (2.0f - h), bad); else sin_a = sqrtf(h * (2.0f - h));
}
// ... and the direction in getCosineWeightedNormal's frame (dir, o1, o2) at the azimuth of u0, with its cosine to nl and the
// factor cosl * (2 * vers) = cosl * Omega / pi
template <bool FAST>
__device__ __forceinline__ void cone_direction(LightSample& out, F3 dir, F3 o1, F3 o2, float cos_a, float sin_a, float vers, float u0, F3 nl, bool& bad,
                                               uint32_t absmask) {
  const float rx = FAST ? u0 * (2.0f * 3.141592654f) : u0 * 2.0f * 3.141592654f;  // doubling is exact (bounce_geometry)
  float sn, cs;
  pt_sincos(rx, sn, cs, absmask);
  const F3 a = o1 * (cs * sin_a);
  const F3 b = o2 * (sn * sin_a);
  const F3 c = dir * cos_a;
  const F3 sum = (a + b) + c;
  if constexpr (FAST) out.l = normalize_nb(sum, bad); else out.l = normalize(sum);
  out.cosl = dot(out.l, nl);
  out.factor = out.cosl * (2.0f * vers);
}

// one sample of the cone the light sphere g = {centre, r * r} subtends at x.  FAST: as in bounce_step
template <bool FAST>
__device__ __forceinline__ LightSample light_sample(F3 x, F3 nl, float4 g, float u0, float u1, bool& bad, uint32_t absmask) {
  LightSample out;
  auto unit = [&](F3 v) { if constexpr (FAST) return normalize_nb(v, bad); else return normalize(v); };
  auto root = [&](float v) { if constexpr (FAST) return sqrt_cr_f32_nb(v, bad); else return sqrtf(v); };
  const F3 sw = mk3(g.x - x.x, g.y - x.y, g.z - x.z);
  const float d2 = dot(sw, sw);
  out.outside = d2 > g.w;
  const float q = g.w / d2;
  const float cmax = root(1.0f - q);
  const float vers = q / (1.0f + cmax);  // 1 - cmax without the cancellation a small lamp would suffer
  float cos_a, sin_a;
  cone_polar<FAST>(u1, vers, cos_a, sin_a, bad);
  // getCosineWeightedNormal's frame (:126-129) around sw
  const F3 dir = unit(sw);
  const F3 o1 = unit(ortho_vector(dir));
  const F3 o2 = unit(cross(dir, o1));
  cone_direction<FAST>(out, dir, o1, o2, cos_a, sin_a, vers, u0, nl, bad, absmask);
  return out;
}

// the sun (EXACTNESS.md A.24): the cone is given, not derived -- the unit direction towards the sun, the frame (o1, o2) the host
// formed around it and vers = 1 - sun_cos; from the polar angle on it is the sphere light's sequence
template <bool FAST>
__device__ __forceinline__ LightSample sun_sample(F3 nl, F3 dir, F3 o1, F3 o2, float vers, float u0, float u1, bool& bad, uint32_t absmask) {
  LightSample out;
  out.outside = true;  // the sun is nowhere
  float cos_a, sin_a;
  cone_polar<FAST>(u1, vers, cos_a, sin_a, bad);
  cone_direction<FAST>(out, dir, o1, o2, cos_a, sin_a, vers, u0, nl, bad, absmask);
  return out;
}

// ---- sky and sun (EXACTNESS.md A.24; tests/sky_model.py is the same definition) -------------------------------------------------
// the radiance an escaping path takes along the unit direction u.  sunned: the previous hit sampled the sun (LIGHTS), so the
// disc is accounted for and the path takes the gradient alone
__device__ __forceinline__ F3 sky_radiance(const PtSkyConsts& sky, F3 u, bool sunned) {
  const F3 grad = mk3(sky.horizon[0] + sky.slope[0] * u.y, sky.horizon[1] + sky.slope[1] * u.y, sky.horizon[2] + sky.slope[2] * u.y);
  F3 rad = u.y >= 0.0f ? grad : mk3(sky.ground[0], sky.ground[1], sky.ground[2]);  // (a NaN takes the ground)
  if (sky.has_sun) {  // wave-uniform
    const bool inside = dot(u, mk3(sky.sun_dir[0], sky.sun_dir[1], sky.sun_dir[2])) >= sky.sun_cos;
    const F3 with_sun = rad + mk3(sky.sun_radiance[0], sky.sun_radiance[1], sky.sun_radiance[2]);
    if (inside & !sunned) rad = with_sun;
  }
  return rad;
}

#ifndef PT_MATERIALS_MIN_WAVES
#define PT_MATERIALS_MIN_WAVES 4  // <= 128 VGPRs
#endif
#ifndef PT_MATERIALS_SKY_MIN_WAVES
#define PT_MATERIALS_SKY_MIN_WAVES 4  // the SKY builds' own bound: they fit the family's without scratch (profiles/sky/README.md)
#endif
// SKY = true takes the sky's constants by value as its third argument (wave-uniform: they are read into scalar registers);
// SKY = false takes the two arguments it always took -- an unused third one would move the hidden arguments that follow the
// explicit ones, and with them an offset inside the instruction stream -- so the third argument is a pack of one or of none
struct NoSky {};
__device__ __forceinline__ NoSky sky_argument() { return NoSky{}; }
__device__ __forceinline__ const PtSkyConsts& sky_argument(const PtSkyConsts& s) { return s; }

template <int RNG, bool LIGHTS, bool SKY, typename... SKY_CONSTS>  // (the LIGHTS builds hold the same bound: 122 / 127 VGPRs, no scratch)
__global__ void __launch_bounds__(PT_BLOCK_THREADS, SKY ? PT_MATERIALS_SKY_MIN_WAVES : PT_MATERIALS_MIN_WAVES)
pixel_kernel_materials(PixelKernelArgs a, const Row* __restrict__ table, SKY_CONSTS... sky_consts) {
  static_assert(sizeof...(SKY_CONSTS) == (SKY ? 1 : 0), "a SKY build takes one PtSkyConsts, the others nothing");
  const auto& sky = sky_argument(sky_consts...);
  extern __shared__ float4 lds_scene[];
  // the table is staged beside the scene image: one slot per sphere after the small tables; stage_scene's barrier covers it
  Row* mtab = reinterpret_cast<Row*>(lds_scene + 4 * a.n_spheres + kTablesF4);
  for (int i = threadIdx.x; i < a.n_spheres; i += blockDim.x) mtab[i] = table[i];
  SceneLds sc = stage_scene<false>(a.spheres, a.n_spheres, lds_scene, false, mk3(a.eye[0], a.eye[1], a.eye[2]), a.spp);
  // the light list: bit i = sphere i emits (any component > 0).  One ballot of the wave over the <= 64 staged spheres, so the
  // list is wave-uniform and lives in scalar registers; light j is its j-th set bit
  uint64_t lights = 0ull;
  if constexpr (LIGHTS) {
    const int li = threadIdx.x & 63;
    bool emits = false;
    if (li < a.n_spheres) {
      const float4 e = sc.mat0[li];
      emits = (e.x > 0.0f) | (e.y > 0.0f) | (e.z > 0.0f);
    }
    lights = __builtin_amdgcn_ballot_w64(emits);
  }

  const uint32_t tp = blockIdx.x * PT_BLOCK_THREADS + threadIdx.x;
  const bool active = tp < a.tile_pixels;  // lanes past the tile stay for the cooperative parts
  const int row = a.row_begin + (int)(tp / (uint32_t)a.width);
  const int col = (int)(tp % (uint32_t)a.width);
  const uint32_t id = (uint32_t)row * (uint32_t)a.width + (uint32_t)col;  // :206

  Rng<RNG> rng;
  if constexpr (RNG == PT_RNG_XORWOW) {
    if (a.rng_state && active) {  // :212
      const uint32_t* s = a.rng_state + (size_t)tp * 6;
      rng.st = Xorwow{s[0], s[1], s[2], s[3], s[4], s[5]};
    } else {
      xorwow_init(rng.st, (uint64_t)id + a.seed);  // :265
    }
  } else {
    rng.k0 = (uint32_t)a.seed;
    rng.k1 = (uint32_t)(a.seed >> 32) ^ a.frame;
    rng.pix = id;
  }
  const F3 B0 = mk3(a.basis[0], a.basis[1], a.basis[2]), B1 = mk3(a.basis[3], a.basis[4], a.basis[5]);
  const F3 B2 = mk3(a.basis[6], a.basis[7], a.basis[8]), B3 = mk3(a.basis[9], a.basis[10], a.basis[11]);
  const F3 eye = mk3(a.eye[0], a.eye[1], a.eye[2]);

  Welford var[4] = {{0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}, {0, 0.0f, 0.0f}};
  TraceOutput L{mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0), 0.0f};

  const int spp = active ? a.spp : 0;
  for (int i = 0; i < spp; i++) {  // :219
    rng.begin_sample((uint32_t)i);
    float sx = (float)row, sy = (float)col;  // :221-229
    if (a.spp != 1) {
      float jx, jy;
      rng.jitter(jx, jy);
      sx += jx * 1.0f - 0.5f;
      sy += jy * 1.0f - 0.5f;
    }
    sx /= (float)a.height;  // contract C7
    sy /= (float)a.width;
    F3 d = lerp(lerp(B0, B1, sy), lerp(B2, B3, sy), 1.0f - sx);
    F3 o = eye;
    F3 color = mk3(0.0f, 0.0f, 0.0f), mask = mk3(1.0f, 1.0f, 1.0f);
    bool escaped = false;
    uint64_t marked = 0ull;  // LIGHTS: bit i = light sphere i was sampled at the previous hit: its emission there is accounted for
    bool sunned = false;     // LIGHTS and SKY: the sun was sampled at the previous hit: an escape now takes the gradient alone
    for (int n = 0; n < a.max_bounces; n++) {  // :155
      float t = 0.0f;
      int idx = 0;
      if (!intersect_scene<6, false, false, false>(sc, a.n_spheres, o, d, t, idx)) {  // :157-161
        escaped = true;
        if constexpr (SKY) {  // the path takes the sky's radiance; a primary ray is not of unit length
          const F3 mr = mask * sky_radiance(sky, n == 0 ? normalize(d) : d, sunned);
          if (n == 0)  // :171-172, applied to the sky as to an emitter seen directly
            color = color + mk3(clampf(mr.x, 0.0f, 1.0f), clampf(mr.y, 0.0f, 1.0f), clampf(mr.z, 0.0f, 1.0f));
          else
            color = color + mr;
        }
        break;
      }
      const float4 g = sc.geom_lane(idx);
      F3 emis, scol;
      float lum_col = 0.0f;
      fetch_material(sc, idx, emis, scol, n == 0 ? &lum_col : nullptr);
      const Row m = mtab[idx];
      float u_az, u_el;
      rng.bounce(n, u_az, u_el);  // for every kind, used or not: the generator's position depends on the bounce number alone
      const F3 centre = mk3(g.x, g.y, g.z);
      bool bad = false;
      Step st = bounce_step<true>(o, d, t, centre, u_az, u_el, m, bad, sc.inv1, sc.absmask);
      if (__builtin_expect(bad, 0)) st = bounce_step<false>(o, d, t, centre, u_az, u_el, m, bad, nullptr, sc.absmask);
      const F3 me = mask * emis;
      F3 lit = color;
      if (n == 0)  // :171-172
        lit = color + mk3(clampf(me.x, 0.0f, 1.0f), clampf(me.y, 0.0f, 1.0f), clampf(me.z, 0.0f, 1.0f));
      else  // :174
        lit = color + me;
      if constexpr (LIGHTS) {
        if (!((marked >> idx) & 1ull)) color = lit;
      } else {
        color = lit;
      }
      mask = mask * scol;  // :175
      mask = mask * st.w;  // GLASS: Re / P or (1 - Re) / (1 - P), after the colour
      if constexpr (LIGHTS) {
        marked = 0ull;
        bool sun_light = false;  // the sun is the LAST light of the list
        if constexpr (SKY) {
          sunned = false;
          sun_light = sky.has_sun != 0;
        }
        if ((lights != 0ull || sun_light) && n < a.max_bounces - 1) {  // wave-uniform; the last bounce does not sample
          const bool diffuse = m.kind == PT_MATERIAL_DIFFUSE;
          uint4 lblk = make_uint4(0u, 0u, 0u, 0u);
          int j = 0;
          for (uint64_t rest = lights; rest != 0ull; rest &= rest - 1ull, j++) {  // a scalar loop
            const int s = __builtin_ctzll(rest);
            float u0, u1;
            light_draws<RNG>(rng, n, j, lblk, u0, u1);  // every path that hit something, whatever the kind
            const float4 lg = sc.geom[s];
            bool lbad = false;
            LightSample ls = light_sample<true>(st.o, st.normal, lg, u0, u1, lbad, sc.absmask);
            bool formed = diffuse & (idx != s) & ls.outside;
            if (__builtin_amdgcn_ballot_w64(formed) == 0ull) continue;
            if (__builtin_expect(formed & lbad, 0)) ls = light_sample<false>(st.o, st.normal, lg, u0, u1, lbad, sc.absmask);
            if (formed) marked |= 1ull << s;  // reached, shadowed or below the horizon: accounted for
            const bool want = formed & (ls.cosl > 0.0f);
            if (__builtin_amdgcn_ballot_w64(want) == 0ull) continue;
            // the same search, the wave converged; a lane without a sample follows its own next ray and its result is dropped
            const F3 sd = want ? ls.l : st.d;
            float shadow_t = 0.0f;
            int shadow_idx = 0;
            const bool shadow_hit = intersect_scene<6, false, false, false>(sc, a.n_spheres, st.o, sd, shadow_t, shadow_idx);
            if (want & shadow_hit & (shadow_idx == s)) {
              const float4 le = sc.mat0[s];
              color = color + (mask * mk3(le.x, le.y, le.z)) * ls.factor;
            }
          }
          if constexpr (SKY) {
            if (sun_light) {  // wave-uniform
              float u0, u1;
              light_draws<RNG>(rng, n, j, lblk, u0, u1);  // light j = the number of emitting spheres
              if (__builtin_amdgcn_ballot_w64(diffuse) != 0ull) {
                const F3 sdir = mk3(sky.sun_dir[0], sky.sun_dir[1], sky.sun_dir[2]);
                const F3 s1 = mk3(sky.sun_o1[0], sky.sun_o1[1], sky.sun_o1[2]), s2 = mk3(sky.sun_o2[0], sky.sun_o2[1], sky.sun_o2[2]);
                bool sbad = false;
                LightSample ls = sun_sample<true>(st.normal, sdir, s1, s2, sky.sun_vers, u0, u1, sbad, sc.absmask);
                if (__builtin_expect(diffuse & sbad, 0)) ls = sun_sample<false>(st.normal, sdir, s1, s2, sky.sun_vers, u0, u1, sbad, sc.absmask);
                sunned = diffuse;  // lit, shadowed or below the horizon: accounted for
                const bool want = diffuse & (ls.cosl > 0.0f);
                if (__builtin_amdgcn_ballot_w64(want) != 0ull) {
                  // the same search, the wave converged, as for a sphere light; lit iff it finds nothing
                  const F3 sd = want ? ls.l : st.d;
                  float shadow_t = 0.0f;
                  int shadow_idx = 0;
                  const bool shadow_hit = intersect_scene<6, false, false, false>(sc, a.n_spheres, st.o, sd, shadow_t, shadow_idx);
                  if (want & !shadow_hit)
                    color = color + (mask * mk3(sky.sun_radiance[0], sky.sun_radiance[1], sky.sun_radiance[2])) * ls.factor;
                }
              }
            }
          }
        }
      }
      if (n == 0) {        // :187-195, from nl, the sphere's colour and t
        L.normal = L.normal + st.normal;
        L.albedo = L.albedo + scol;
        L.depth += t;
        welford_update3(var[1], var[2], var[3], luminance(st.normal), lum_col, t, sc.rcpn);
      }
      o = st.o;
      d = st.d;
    }
    L.color = L.color + color;  // :159 / :198
    // :200 -- and the decision of A.24: under a sky the escaped paths carry light, so EVERY sample counts
    if (SKY || !escaped) welford_update(var[0], luminance(color), sc.rcpn);
  }

  float px[14];
  frame_values(L, var, (float)a.spp, px);  // :234-254
  if (a.vertices && active) store_display_vertex(a.vertices + (size_t)tp * 3, a.width, row, col, px[0], px[1], px[2]);
  if (a.planar) {
    if (active) {
#pragma unroll
      for (int c = 0; c < 14; c++) a.out[(size_t)c * a.tile_pixels + tp] = px[c];
    }
  } else {
    // a full wave's 64 pixels are one contiguous 3584-byte span: transpose through the wave's LDS slice, 16-byte stores
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool wave_full = (__builtin_amdgcn_ballot_w64(active) == ~0ull) && ((reinterpret_cast<uintptr_t>(a.out) & 15u) == 0u);
    if (wave_full) {
      float* wl = reinterpret_cast<float*>(lds_scene + a.scene_lds_f4) + wave * (64 * 14);
#pragma unroll
      for (int c = 0; c < 14; c++) wl[lane * 14 + c] = px[c];
      __builtin_amdgcn_wave_barrier();
      const float4* src = reinterpret_cast<const float4*>(wl);
      float4* dst = reinterpret_cast<float4*>(a.out + (size_t)(tp - (uint32_t)lane) * 14);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int q = lane + 64 * k;
        if (q < 224) dst[q] = src[q];
      }
    } else if (active) {
      float* op = a.out + (size_t)tp * 14;
#pragma unroll
      for (int c = 0; c < 14; c++) op[c] = px[c];
    }
  }
  if constexpr (RNG == PT_RNG_XORWOW) {
    if (a.rng_state && active) {  // :256
      uint32_t* s = a.rng_state + (size_t)tp * 6;
      s[0] = rng.st.d; s[1] = rng.st.v0; s[2] = rng.st.v1; s[3] = rng.st.v2; s[4] = rng.st.v3; s[5] = rng.st.v4;
    }
  }
}

}  // namespace materials
}  // namespace pt

typedef void (*materials_kernel_fn)(PixelKernelArgs, const pt::materials::Row*);
typedef void (*materials_sky_kernel_fn)(PixelKernelArgs, const pt::materials::Row*, PtSkyConsts);

static materials_kernel_fn select_materials(int rng_mode, bool lights) {
  using namespace pt::materials;
  if (lights) return rng_mode == PT_RNG_PHILOX ? pixel_kernel_materials<PT_RNG_PHILOX, true, false> : pixel_kernel_materials<PT_RNG_XORWOW, true, false>;
  return rng_mode == PT_RNG_PHILOX ? pixel_kernel_materials<PT_RNG_PHILOX, false, false> : pixel_kernel_materials<PT_RNG_XORWOW, false, false>;
}

static materials_sky_kernel_fn select_materials_sky(int rng_mode, bool lights) {
  using namespace pt::materials;
  if (lights) return rng_mode == PT_RNG_PHILOX ? pixel_kernel_materials<PT_RNG_PHILOX, true, true, PtSkyConsts> : pixel_kernel_materials<PT_RNG_XORWOW, true, true, PtSkyConsts>;
  return rng_mode == PT_RNG_PHILOX ? pixel_kernel_materials<PT_RNG_PHILOX, false, true, PtSkyConsts> : pixel_kernel_materials<PT_RNG_XORWOW, false, true, PtSkyConsts>;
}

const void* pt_materials_kernel_symbol(int rng_mode, bool lights, bool sky) {
  return sky ? (const void*)select_materials_sky(rng_mode, lights) : (const void*)select_materials(rng_mode, lights);
}

static uint32_t materials_scene_f4(int n_spheres) { return (uint32_t)n_spheres * 5u + (uint32_t)pt::kTablesF4; }  // scene image, small tables, table

size_t pt_materials_kernel_lds_bytes(int n_spheres) {
  return (size_t)materials_scene_f4(n_spheres) * sizeof(float4) + (PT_BLOCK_THREADS / 64) * 64 * 14 * sizeof(float);
}

// a pt_material as the kernel reads it; 1 / eta and R0 are formed here, in float32, one rounding per operation
void pt_materials_device_row(const pt_material* m, void* row16) {
  pt::materials::Row r{m->kind, m->param, 0.0f, 0.0f};
  if (m->kind == PT_MATERIAL_GLASS) {
    const float eta = m->param;
    const float em = eta - 1.0f, ep = eta + 1.0f;
    r.inv = 1.0f / eta;
    r.r0 = (em * em) / (ep * ep);
  }
  memcpy(row16, &r, sizeof(r));
}

// the sky's constants as the kernel reads them (EXACTNESS.md A.24): slope = zenith - horizon; with a sun the unit direction
// v * (1 / sqrt(dot(v, v))), getCosineWeightedNormal's frame around it and vers = 1 - sun_cos -- float32, one rounding per operation
void pt_materials_sky_consts(const pt_sky* s, PtSkyConsts* out) {
  PtSkyConsts c;
  memset(&c, 0, sizeof(c));
  for (int k = 0; k < 3; k++) {
    c.horizon[k] = s->horizon[k];
    c.slope[k] = s->zenith[k] - s->horizon[k];
    c.ground[k] = s->ground[k];
    c.sun_radiance[k] = s->sun_radiance[k];
  }
  c.has_sun = (s->sun_radiance[0] > 0.0f) | (s->sun_radiance[1] > 0.0f) | (s->sun_radiance[2] > 0.0f);
  if (c.has_sun) {
    auto unit = [](const float* v, float* o) {
      const float inv = 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int k = 0; k < 3; k++) o[k] = v[k] * inv;
    };
    unit(s->sun_dir, c.sun_dir);
    const float* d = c.sun_dir;
    const float zero = 0.0f;
    const float ortho[3] = {fabsf(d[0]) > fabsf(d[2]) ? -d[1] : zero, fabsf(d[0]) > fabsf(d[2]) ? d[0] : -d[2], fabsf(d[0]) > fabsf(d[2]) ? zero : d[1]};
    unit(ortho, c.sun_o1);
    const float* p = c.sun_o1;
    const float cr[3] = {d[1] * p[2] - d[2] * p[1], d[2] * p[0] - d[0] * p[2], d[0] * p[1] - d[1] * p[0]};
    unit(cr, c.sun_o2);
    c.sun_cos = s->sun_cos;
    c.sun_vers = 1.0f - s->sun_cos;
  }
  *out = c;
}

hipError_t pt_launch_materials_kernel(const PixelKernelArgs& a, const void* d_table, int rng_mode, bool lights, const PtSkyConsts* sky,
                                      hipStream_t stream) {
  PixelKernelArgs b = a;
  b.scene_lds_f4 = materials_scene_f4(a.n_spheres);
  const unsigned grid = (unsigned)(((uint64_t)a.tile_pixels + PT_BLOCK_THREADS - 1) / PT_BLOCK_THREADS);
  if (sky) {
    hipLaunchKernelGGL(select_materials_sky(rng_mode, lights), dim3(grid), dim3(PT_BLOCK_THREADS), pt_materials_kernel_lds_bytes(a.n_spheres), stream,
                       b, (const pt::materials::Row*)d_table, *sky);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(select_materials(rng_mode, lights), dim3(grid), dim3(PT_BLOCK_THREADS), pt_materials_kernel_lds_bytes(a.n_spheres), stream, b,
                     (const pt::materials::Row*)d_table);
  return hipGetLastError();  // (outside the launch census: no PT_LAUNCHED)
}
