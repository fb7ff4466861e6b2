// exr_reader_check.cpp -- drives host/ExrReader.h for tests/test_exr_reader_host.py; host code only.
//   decode FILE OUT      decodes FILE, prints "width height present-mask", writes the buffer [h][w][14] as raw floats to OUT;
//                        a refusal prints the reader's message to stderr and exits 3
//   golden FILE W H MODE FILE decodes to writer_check.cpp's pattern of that size (bit for bit)
//   roundtrip W H SEED   EncodeFeatureEXR -> DecodeFeatureEXR is the identity on W x H x 14 random bit patterns
//   fuzz                 a 4 x 3 file truncated at every length, and with every bit of every header byte flipped in turn: every
//                        call returns (a refusal or a decode); built with the sanitizers, which must stay silent
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ExrReader.h"

static float pattern(int i, int mode) {
  if (mode == 0) return (float)i;
  return 1.3f * sinf(0.37f * (float)i) + 0.002f * (float)(i % 97);
}

static std::vector<float> random_buffer(int width, int height, uint64_t seed) {
  std::vector<float> buffer((size_t)width * height * 14);
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  for (size_t i = 0; i < buffer.size(); i++) {  // every bit pattern: NaN and inf among them
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    const uint32_t u = (uint32_t)(s >> 16);
    memcpy(&buffer[i], &u, 4);
  }
  return buffer;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  ptexr::FeatureImage img;
  std::string err;
  if (mode == "decode" && argc == 4) {
    if (!ptexr::LoadFeatureEXR(argv[2], &img, &err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 3;
    }
    unsigned mask = 0;
    for (int k = 0; k < 14; k++) mask |= (img.present[k] ? 1u : 0u) << k;
    printf("%d %d %u\n", img.width, img.height, mask);
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 1;
    const bool ok = fwrite(img.buffer.data(), sizeof(float), img.buffer.size(), f) == img.buffer.size();
    return fclose(f) == 0 && ok ? 0 : 1;
  }
  if (mode == "golden" && argc == 6) {
    const int width = atoi(argv[3]), height = atoi(argv[4]), pat = atoi(argv[5]);
    if (!ptexr::LoadFeatureEXR(argv[2], &img, &err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 3;
    }
    std::vector<float> want((size_t)width * height * 14);
    for (size_t i = 0; i < want.size(); i++) want[i] = pattern((int)i, pat);
    for (int k = 0; k < 14; k++)
      if (!img.present[k]) return 4;
    return img.width == width && img.height == height && same_bits(img.buffer, want) ? 0 : 5;
  }
  if (mode == "roundtrip" && argc == 5) {
    const int width = atoi(argv[2]), height = atoi(argv[3]);
    const std::vector<float> buffer = random_buffer(width, height, (uint64_t)atoll(argv[4]));
    const std::vector<unsigned char> bytes = ptexr::EncodeFeatureEXR(buffer.data(), width, height);
    if (!ptexr::DecodeFeatureEXR(bytes.data(), bytes.size(), &img, &err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 3;
    }
    return img.width == width && img.height == height && same_bits(img.buffer, buffer) ? 0 : 5;
  }
  if (mode == "fuzz") {
    const int width = 4, height = 3;
    const std::vector<float> buffer = random_buffer(width, height, 7);
    const std::vector<unsigned char> bytes = ptexr::EncodeFeatureEXR(buffer.data(), width, height);
    const size_t header = bytes.size() - (size_t)height * (8 + 8 + (size_t)width * 14 * 4);  // (what precedes the offset table)
    int refused = 0, decoded = 0;
    for (size_t n = 0; n <= bytes.size(); n++) {
      std::vector<unsigned char> cut(bytes.begin(), bytes.begin() + n);  // (its own allocation: an overrun is seen)
      if (ptexr::DecodeFeatureEXR(cut.data(), cut.size(), &img, &err)) {
        if (n != bytes.size() || !same_bits(img.buffer, buffer)) return 5;  // only the whole file decodes
        decoded++;
      } else {
        if (err.empty()) return 6;
        refused++;
      }
    }
    printf("truncated: %d refused, %d decoded\n", refused, decoded);
    refused = decoded = 0;
    for (size_t i = 0; i < header + (size_t)height * 8; i++)  // the header and the offset table
      for (int bit = 0; bit < 8; bit++) {
        std::vector<unsigned char> bad(bytes);
        bad[i] ^= (unsigned char)(1u << bit);
        if (ptexr::DecodeFeatureEXR(bad.data(), bad.size(), &img, &err)) {
          if (img.width <= 0 || img.height <= 0 || img.buffer.size() != (size_t)img.width * img.height * 14) return 7;
          decoded++;
        } else {
          if (err.empty()) return 6;
          refused++;
        }
      }
    printf("flipped: %d refused, %d decoded\n", refused, decoded);
    return 0;
  }
  fprintf(stderr, "usage: exr_reader_check decode FILE OUT | golden FILE W H MODE | roundtrip W H SEED | fuzz\n");
  return 2;
}
