// Sky.h -- the sky of `pathtrace --sky FILE | clear` (no counterpart in the reference, where a ray that leaves the scene returns
// nothing: src/pathtrace.cu:157-161).  A file holds lines "zenith r g b", "horizon r g b", "ground r g b" and
// "sun dx dy dz cos r g b" (direction TOWARDS the sun, cosine of its angular radius, radiance of the disc), each at most once;
// blank lines and lines that start with '#' are skipped; unlisted lines are zero.  "clear" is the preset of a clear day, the
// Python package's CLEAR_SKY.  Host code only: parsing needs no device, the values are checked by the library's own pt_sky_check,
// and every refusal comes before a device is touched.
#ifndef SKY_H
#define SKY_H
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "pathtrace.h"

typedef pt_sky Sky;

// a blue-to-white gradient, a grey ground, a sun of angular radius 2.56 degrees 64 degrees above the horizon
inline Sky ClearSky() {
  Sky s;
  memset(&s, 0, sizeof(s));
  const float zenith[3] = {0.18f, 0.36f, 0.80f}, horizon[3] = {0.80f, 0.85f, 0.90f}, ground[3] = {0.25f, 0.25f, 0.25f};
  const float dir[3] = {0.4f, 0.8f, 0.45f}, radiance[3] = {400.0f, 380.0f, 340.0f};
  for (int k = 0; k < 3; k++) {
    s.zenith[k] = zenith[k];
    s.horizon[k] = horizon[k];
    s.ground[k] = ground[k];
    s.sun_dir[k] = dir[k];
    s.sun_radiance[k] = radiance[k];
  }
  s.sun_cos = 0.999f;
  return s;
}

// false: `error` says why (an unreadable file, an unknown key, a key given twice, a line with too few or too many numbers or
// with something that is no number, a file without any line, whatever pt_sky_check refuses)
inline bool ParseSky(const std::string& file, Sky& out, std::string& error) {
  memset(&out, 0, sizeof(out));
  std::ifstream in(file.c_str());
  if (!in) {
    error = "cannot open sky file " + file;
    return false;
  }
  static const char* const keys[4] = {"zenith", "horizon", "ground", "sun"};
  static const int counts[4] = {3, 3, 3, 7};
  bool seen[4] = {false, false, false, false};
  std::string line;
  int number = 0, listed = 0;
  while (std::getline(in, line)) {
    number++;
    const size_t first = line.find_first_not_of(" \t\r");
    if (first == std::string::npos || line[first] == '#') continue;
    std::ostringstream where;
    where << file << " line " << number << ": ";
    std::istringstream ls(line);
    std::string key, word;
    ls >> key;
    int which = -1;
    for (int k = 0; k < 4; k++)
      if (key == keys[k]) which = k;
    if (which < 0) {
      error = where.str() + "key '" + key + "' is none of zenith, horizon, ground, sun";
      return false;
    }
    if (seen[which]) {
      error = where.str() + "'" + key + "' is repeated";
      return false;
    }
    seen[which] = true;
    float v[7] = {0, 0, 0, 0, 0, 0, 0};
    int n = 0;
    bool ok = true;
    while (ok && (ls >> word)) {  // (strtod, so that "nan" and "inf" are read and refused as what they are)
      char* end = NULL;
      const double x = strtod(word.c_str(), &end);
      ok = end != word.c_str() && *end == '\0' && n < counts[which];
      if (ok) v[n++] = (float)x;
    }
    if (!ok || n != counts[which]) {
      error = where.str() + (which == 3 ? "expected 'sun dx dy dz cos r g b'" : "expected '" + key + " r g b'");
      return false;
    }
    float* const dst = which == 0 ? out.zenith : which == 1 ? out.horizon : which == 2 ? out.ground : out.sun_dir;
    for (int k = 0; k < 3; k++) dst[k] = v[k];
    if (which == 3) {
      out.sun_cos = v[3];
      for (int k = 0; k < 3; k++) out.sun_radiance[k] = v[4 + k];
    }
    listed++;
  }
  if (listed == 0) {
    error = "no sky in " + file;
    return false;
  }
  if (pt_sky_check(&out) != PT_OK) {
    error = file + ": " + pt_last_error();
    return false;
  }
  return true;
}
#endif
