// Velocities.h -- the velocity list of `pathtrace --velocities FILE` (no counterpart in the reference, whose scene is at rest).
// One line per moving sphere: "index vx vy vz"; blank lines and lines that start with '#' are skipped.  In frame k sphere `index`
// has the centre pos0 + (float)k * v, per component in float32 (build without contraction).  Host code only: parsing and the
// per-frame scene need no device, and every refusal comes before one is touched.
#ifndef VELOCITIES_H
#define VELOCITIES_H
#include <errno.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "Scene.h"

struct SphereVelocity {
  int index;
  float v[3];
};

// false: `error` says why (an unreadable file, a malformed line, an index outside 0 .. nSpheres - 1 or given twice, a number that
// is not finite).  An empty list is an error too: the flag would do nothing.
inline bool ParseVelocities(const std::string& file, int nSpheres, std::vector<SphereVelocity>& out, std::string& error) {
  out.clear();
  std::ifstream in(file.c_str());
  if (!in) {
    error = "cannot open velocity file " + file;
    return false;
  }
  std::vector<bool> seen(nSpheres > 0 ? (size_t)nSpheres : 0, false);
  std::string line;
  int number = 0;
  while (std::getline(in, line)) {
    number++;
    const size_t first = line.find_first_not_of(" \t\r");
    if (first == std::string::npos || line[first] == '#') continue;
    std::ostringstream where;
    where << file << " line " << number << ": ";
    std::istringstream ls(line);
    long long index = 0;
    double v[3];
    std::string first_word, word[3], extra;
    bool ok = static_cast<bool>(ls >> first_word >> word[0] >> word[1] >> word[2]) && !(ls >> extra);
    if (ok) {  // (the whole word must be an integer: "7.5 1 0 0" is not index 7 with another velocity)
      char* end = NULL;
      errno = 0;
      index = strtoll(first_word.c_str(), &end, 10);
      ok = end != first_word.c_str() && *end == '\0' && errno == 0;
    }
    for (int k = 0; ok && k < 3; k++) {  // (strtod, so that "nan" and "inf" are read and refused as what they are)
      char* end = NULL;
      v[k] = strtod(word[k].c_str(), &end);
      ok = end != word[k].c_str() && *end == '\0';
    }
    if (!ok) {
      error = where.str() + "expected 'index vx vy vz'";
      return false;
    }
    if (index < 0 || index >= nSpheres) {
      std::ostringstream m;
      m << where.str() << "index " << index << " outside 0 .. " << nSpheres - 1;
      error = m.str();
      return false;
    }
    if (seen[(size_t)index]) {
      std::ostringstream m;
      m << where.str() << "index " << index << " is repeated";
      error = m.str();
      return false;
    }
    seen[(size_t)index] = true;
    SphereVelocity s;
    s.index = (int)index;
    for (int k = 0; k < 3; k++) {
      if (!(v[k] >= -3.4028234663852886e38 && v[k] <= 3.4028234663852886e38)) {
        error = where.str() + "a velocity component is not a finite float";
        return false;
      }
      s.v[k] = (float)v[k];
    }
    out.push_back(s);
  }
  if (out.empty()) {
    error = "no velocities in " + file;
    return false;
  }
  return true;
}

// The scene of frame k.
inline void MoveSpheres(const std::vector<Sphere>& at0, const std::vector<SphereVelocity>& velocities, int k, std::vector<Sphere>& out) {
  out = at0;
  const float fk = (float)k;
  for (size_t i = 0; i < velocities.size(); i++) {
    Sphere& s = out[(size_t)velocities[i].index];
    const float dx = fk * velocities[i].v[0], dy = fk * velocities[i].v[1], dz = fk * velocities[i].v[2];
    s.pos.x = s.pos.x + dx, s.pos.y = s.pos.y + dy, s.pos.z = s.pos.z + dz;
  }
}
#endif
