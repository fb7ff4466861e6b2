// Material.h -- the material table of `pathtrace --materials FILE | smallpt` (no counterpart in the reference, which renders diffuse
// surfaces only).  One line per sphere that is not diffuse: "index kind [param]", kind = diffuse | mirror | glossy | glass or
// 0 .. 3; blank lines and lines that start with '#' are skipped; unlisted spheres are diffuse.  "smallpt" is the preset of
// smallpt's Cornell box: sphere 6 a mirror ball, sphere 7 a glass ball of index 1.5.  Host code only: parsing needs no device, the
// values are checked by the library's own pt_material_check, and every refusal comes before a device is touched.
#ifndef MATERIAL_H
#define MATERIAL_H
#include <errno.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pathtrace.h"

// the preset needs the reference's nine spheres
inline bool SmallptMaterials(int nSpheres, std::vector<pt_material>& out, std::string& error) {
  if (nSpheres != 9) {
    error = "the smallpt preset is for the reference's scene of 9 spheres";
    return false;
  }
  out.assign(9, pt_material{PT_MATERIAL_DIFFUSE, 0.0f});
  out[6] = pt_material{PT_MATERIAL_MIRROR, 0.0f};
  out[7] = pt_material{PT_MATERIAL_GLASS, 1.5f};
  return true;
}

// false: `error` says why (an unreadable file, a malformed line, an unknown kind, an index outside 0 .. nSpheres - 1 or given
// twice, whatever pt_material_check refuses).  An empty list is an error too: the flag would do nothing.
inline bool ParseMaterials(const std::string& file, int nSpheres, std::vector<pt_material>& out, std::string& error) {
  out.assign(nSpheres > 0 ? (size_t)nSpheres : 0, pt_material{PT_MATERIAL_DIFFUSE, 0.0f});
  std::ifstream in(file.c_str());
  if (!in) {
    error = "cannot open material file " + file;
    return false;
  }
  static const char* const names[4] = {"diffuse", "mirror", "glossy", "glass"};
  std::vector<bool> seen(out.size(), false);
  std::string line;
  int number = 0, listed = 0;
  while (std::getline(in, line)) {
    number++;
    const size_t first = line.find_first_not_of(" \t\r");
    if (first == std::string::npos || line[first] == '#') continue;
    std::ostringstream where;
    where << file << " line " << number << ": ";
    std::istringstream ls(line);
    std::string index_word, kind_word, param_word, extra;
    bool ok = static_cast<bool>(ls >> index_word >> kind_word);
    const bool has_param = ok && static_cast<bool>(ls >> param_word);
    ok = ok && !(ls >> extra);
    long long index = 0;
    if (ok) {
      char* end = NULL;
      errno = 0;
      index = strtoll(index_word.c_str(), &end, 10);
      ok = end != index_word.c_str() && *end == '\0' && errno == 0;
    }
    double param = 0.0;
    if (ok && has_param) {  // (strtod, so that "nan" and "inf" are read and refused as what they are)
      char* end = NULL;
      param = strtod(param_word.c_str(), &end);
      ok = end != param_word.c_str() && *end == '\0';
    }
    if (!ok) {
      error = where.str() + "expected 'index kind [param]'";
      return false;
    }
    int kind = -1;
    for (int k = 0; k < 4; k++)
      if (kind_word == names[k] || (kind_word.size() == 1 && kind_word[0] == '0' + k)) kind = k;
    if (kind < 0) {
      error = where.str() + "kind '" + kind_word + "' is none of diffuse, mirror, glossy, glass (0 .. 3)";
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
    out[(size_t)index] = pt_material{kind, (float)param};  // (a double beyond float is inf here: refused below as not finite)
    listed++;
  }
  if (listed == 0) {
    error = "no materials in " + file;
    return false;
  }
  if (pt_material_check(out.data(), (int)out.size()) != PT_OK) {
    error = file + ": " + pt_last_error();
    return false;
  }
  return true;
}
#endif
