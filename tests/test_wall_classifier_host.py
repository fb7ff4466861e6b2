"""The wall classifier's equality rule on the host (csrc/pt_walls.h is plain C++ behind __host__ __device__): the two walls of
an axis must carry the same BITS in the two coordinates off their axis, or the scene is declined (EXACTNESS.md A.21).  The GPU
tests can only see that a declined scene still renders exactly; this one sees the decision."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r"""
#define __host__
#define __device__
#include <cstdio>
#include <cstring>
#include "cuda-pathtrace_amd/csrc/pt_walls.h"
static pt_sphere wall(float r, float x, float y, float z) {
  pt_sphere s;
  memset(&s, 0, sizeof s);
  s.radius = r; s.pos[0] = x; s.pos[1] = y; s.pos[2] = z;
  return s;
}
static float next_up(float x) { unsigned u; memcpy(&u, &x, 4); u += 1; memcpy(&x, &u, 4); return x; }
int main() {
  // a box about the origin (every point of it inside all six huge spheres): the shared coordinates are zeros, so that the sign of a zero can be one of the cases
  pt_sphere base[9] = {wall(1e5f, -1e5f + 50, 0, 0), wall(1e5f, 1e5f - 50, 0, 0), wall(1e5f, 0, -1e5f + 40, 0), wall(1e5f, 0, 1e5f - 40, 0),
                       wall(1e5f, 0, 0, -1e5f + 80), wall(1e5f, 0, 0, 1e5f - 80), wall(16.5f, -23, -24, -30), wall(16.5f, 23, -24, 10),
                       wall(6.f, 0, 30, 0)};
  printf("base %d\n", (int)pt::classify_walls(base, 9).ok);
  for (int w = 0; w < 6; w++)
    for (int j = 0; j < 3; j++) {
      if (j == w / 2) continue;
      pt_sphere s[9];
      memcpy(s, base, sizeof s);
      s[w].pos[j] = -0.0f;  // equal in value to the partner's +0, not in bits
      printf("negzero %d %d %d\n", w, j, (int)pt::classify_walls(s, 9).ok);
      memcpy(s, base, sizeof s);
      s[w].pos[j] = 1.4e-45f;  // one ulp above the partner's +0
      printf("ulp %d %d %d\n", w, j, (int)pt::classify_walls(s, 9).ok);
    }
  pt_sphere s[9];
  memcpy(s, base, sizeof s);
  for (int w = 0; w < 6; w++) s[w].pos[(w / 2 + 1) % 3] = next_up(7.3f);  // moved together, differently per pair: still a box
  printf("together %d\n", (int)pt::classify_walls(s, 9).ok);
  return 0;
}
"""


def test_pairs_must_agree_in_bits_off_their_axis(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "walls.cpp", tmp_path / "walls"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", ROOT, str(src), "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.split("\n")
    got = {tuple(l.split()[:-1]): int(l.split()[-1]) for l in out if l}
    assert got.pop(("base",)) == 1 and got.pop(("together",)) == 1, out
    assert len(got) == 24 and not any(got.values()), got  # 6 walls x 2 shared coordinates x {-0, one ulp}: all declined
