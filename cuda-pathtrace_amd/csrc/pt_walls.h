// pt_walls.h -- the axis walls of a nine-sphere scene, decided once per workgroup from the scene's own floats.
//
// A Cornell box built of spheres (Scene.h:26-31) has six "axis walls": spheres whose radius dwarfs the scene and whose centre lies
// off the box along exactly one axis, one on each side of each axis.  Every point of the box is inside all six, so a ray can only
// reach, on each axis, the wall of the pair it points toward: the other root of the other wall is the far side of a huge sphere.
// The secondary-bounce screen (intersect_scene_screened_keys, EXACTNESS.md A.18) ranks the faced wall of each axis and certifies
// the other one instead of screening it.  The certificate is sound for ANY sphere, so this classification only decides how often
// it passes: a scene without the structure gets a layout that never certifies (ok = false) and every sphere is screened.
// The screen also takes the behind wall's two off-axis offsets from the faced wall of the pair (screen_walled, EXACTNESS.md
// A.21), so "the structure" includes that the two centres of a pair carry the same bits off their axis.
#pragma once
#include <math.h>
#include "../../include/ptcore.h"

namespace pt {

struct WallLayout {
  int obj[3];    // the three spheres that are always screened
  int minus[3];  // per axis: the wall whose centre lies on the minus side (faced by a ray with d[axis] >= 0)
  int plus[3];   // per axis: the wall whose centre lies on the plus side (faced by a ray with d[axis] < 0)
  bool ok;       // the scene has the structure: the behind walls may be certified
};

// n must be 9 for any structure; every other scene (and every rejected one) gets the identity-like layout with ok = false,
// which still covers each sphere exactly once per lane: objects 6, 7, 8, and per axis the pair {2k, 2k + 1}.
__host__ __device__ inline WallLayout classify_walls(const pt_sphere* s, int n) {
  WallLayout w{{6, 7, 8}, {0, 2, 4}, {1, 3, 5}, false};
  const WallLayout none = w;
  if (n != 9) return w;
  double rmax = 0.0;
  for (int i = 0; i < 9; i++) {
    const double r = (double)s[i].radius;
    if (!(r >= 0.0) || !(r < 1e30)) return none;  // NaN, negative or infinite radius
    rmax = r > rmax ? r : rmax;
  }
  // the wall candidates: the spheres of at least half the largest radius -- exactly six of them
  int walls[6], objs[3], nw = 0, no = 0;
  for (int i = 0; i < 9; i++) {
    if ((double)s[i].radius >= 0.5 * rmax) {
      if (nw == 6) return none;
      walls[nw++] = i;
    } else {
      if (no == 3) return none;
      objs[no++] = i;
    }
  }
  if (nw != 6 || no != 3) return none;
  // reference point: the mean of the six wall centres (each pair's huge offsets cancel along its axis)
  double p[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < 6; j++)
    for (int k = 0; k < 3; k++) p[k] += (double)s[walls[j]].pos[k] / 6.0;
  double ext = 0.0;  // how far the other spheres' centres lie from it
  for (int j = 0; j < 3; j++)
    for (int k = 0; k < 3; k++) {
      const double e = fabs((double)s[objs[j]].pos[k] - p[k]);
      if (!(e < 1e30)) return none;
      ext = e > ext ? e : ext;
    }
  int mi[3] = {-1, -1, -1}, pl[3] = {-1, -1, -1};
  for (int j = 0; j < 6; j++) {
    const pt_sphere& sw = s[walls[j]];
    const double r = (double)sw.radius;
    if (sw.emission[0] != 0.0f || sw.emission[1] != 0.0f || sw.emission[2] != 0.0f) return none;  // an emitting wall
    if (!(r >= 100.0 * ext) || !(r > 0.0)) return none;  // not huge next to the rest of the scene
    double off[3];
    int ax = 0;
    for (int k = 0; k < 3; k++) {
      off[k] = (double)sw.pos[k] - p[k];
      if (!(fabs(off[k]) < 1e30)) return none;
      if (fabs(off[k]) > fabs(off[ax])) ax = k;
    }
    if (!(fabs(off[ax]) >= 0.5 * r)) return none;  // the centre must lie off the box ...
    for (int k = 0; k < 3; k++)
      if (k != ax && !(fabs(off[k]) <= 1e-2 * r)) return none;  // ... along exactly one axis (a tilted centre breaks this)
    int* slot = off[ax] > 0.0 ? &pl[ax] : &mi[ax];
    if (*slot >= 0) return none;  // two walls on one side of one axis: nested or duplicated
    *slot = walls[j];
  }
  for (int k = 0; k < 3; k++) {
    if (mi[k] < 0 || pl[k] < 0) return none;  // a missing wall
    // the two walls' insides overlap along the axis: the plus wall's near surface lies below the minus wall's
    const pt_sphere &a = s[pl[k]], &b = s[mi[k]];
    if (!((double)a.pos[k] - (double)a.radius < (double)b.pos[k] + (double)b.radius)) return none;
    // the two centres differ along their axis ONLY: the screen forms o - centre, its square and its product with d for the
    // other two coordinates once per pair (screen_walled, EXACTNESS.md A.21), which is the same float only for the same BITS
    // (+0 and -0 are equal values and give o - c different signs of zero)
    for (int j = 0; j < 3; j++)
      if (j != k && __builtin_bit_cast(unsigned, a.pos[j]) != __builtin_bit_cast(unsigned, b.pos[j])) return none;
  }
  for (int k = 0; k < 3; k++) {
    w.obj[k] = objs[k];
    w.minus[k] = mi[k];
    w.plus[k] = pl[k];
  }
  w.ok = true;
  return w;
}

}  // namespace pt
