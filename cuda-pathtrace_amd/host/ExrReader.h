// ExrReader.h -- the inverse of ExrWriter.h: reads the 14-channel float32 EXR that OutputBuffer::SaveEXR writes (and the
// reference writes through tinyexr) back into an interleaved buffer[row][col][14].  Written from the file format, for exactly
// that subset: a single-part scanline file, every channel FLOAT with sampling 1, compression NONE, a data window that starts
// at (0, 0), increasing line order; attributes in any order.  Color.R/G/B are required; any other of the 14 known channels is
// filled in when present and zero otherwise, and channels with other names are skipped.  The line-offset table is honoured, and
// every offset and length is checked against the size of the file before it is used.  Everything else (a compression, HALF or
// UINT channels, tiles, multipart, deep data, a truncated file) is refused with a message naming what was found.  Header only,
// host code only.
#ifndef PT_EXR_READER_H
#define PT_EXR_READER_H
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ExrWriter.h"

namespace ptexr {

struct FeatureImage {
  int width, height;
  std::vector<float> buffer;  // [height][width][14]
  bool present[14];           // by buffer index: the file had the channel
  FeatureImage() : width(0), height(0) { memset(present, 0, sizeof(present)); }
};

namespace detail {

struct Cursor {
  const unsigned char* p;
  size_t size, at;
  bool u32(uint32_t* v) {
    if (size - at < 4) return false;
    *v = (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
    at += 4;
    return true;
  }
  // a NUL-terminated string of 1 .. 255 bytes ("" is returned as empty with ok = true)
  bool str(std::string* s) {
    s->clear();
    while (at < size && p[at] != 0 && s->size() < 256) s->push_back((char)p[at++]);
    if (at >= size || p[at] != 0) return false;
    at++;
    return true;
  }
};

inline uint32_t le32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t le64(const unsigned char* p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

inline bool refuse(std::string* err, const std::string& what) {
  if (err) *err = what;
  return false;
}
inline std::string num(long long v) {
  char text[32];
  snprintf(text, sizeof(text), "%lld", v);
  return text;
}

}  // namespace detail

inline bool DecodeFeatureEXR(const unsigned char* bytes, size_t size, FeatureImage* out, std::string* err) {
  using namespace detail;
  if (!out || (!bytes && size)) return refuse(err, "Invalid argument.");
  *out = FeatureImage();
  if (size < 8) return refuse(err, "truncated file: " + num((long long)size) + " bytes hold no EXR header");
  if (le32(bytes) != 0x01312f76u) return refuse(err, "not an EXR file: magic " + num(le32(bytes)));
  const uint32_t version = le32(bytes + 4);
  if ((version & 0xffu) != 2) return refuse(err, "EXR version " + num(version & 0xffu) + " (only 2 is read)");
  if (version & 0x200u) return refuse(err, "a tiled file (only scanline files are read)");
  if (version & 0x800u) return refuse(err, "a deep-data file (only flat scanline files are read)");
  if (version & 0x1000u) return refuse(err, "a multipart file (only single-part files are read)");
  if (version & ~0xffu) return refuse(err, "version flags " + num(version >> 8) + " (none are read)");

  Cursor c = {bytes, size, 8};
  std::vector<int> slots;  // per channel of the file, in file order: the buffer index, or -1 for a name that is not ours
  bool have_channels = false, have_compression = false, have_window = false;
  int64_t width = 0, height = 0;
  for (;;) {
    std::string name, type;
    if (!c.str(&name)) return refuse(err, "truncated file: the header ends inside an attribute name at byte " + num((long long)c.at));
    if (name.empty()) break;
    uint32_t len = 0;
    if (!c.str(&type) || !c.u32(&len)) return refuse(err, "truncated file: the header ends inside attribute '" + name + "'");
    if (len > size - c.at) return refuse(err, "truncated file: attribute '" + name + "' of " + num(len) + " bytes runs past the end");
    Cursor v = {bytes, c.at + len, c.at};
    c.at += len;
    if (name == "channels") {
      if (type != "chlist") return refuse(err, "attribute 'channels' of type '" + type + "'");
      if (have_channels) return refuse(err, "a second 'channels' attribute");
      have_channels = true;
      for (;;) {
        std::string ch;
        if (!v.str(&ch)) return refuse(err, "attribute 'channels' ends inside a channel name");
        if (ch.empty()) break;
        uint32_t pixel_type = 0, linear = 0, xs = 0, ys = 0;
        if (!v.u32(&pixel_type) || !v.u32(&linear) || !v.u32(&xs) || !v.u32(&ys))
          return refuse(err, "attribute 'channels' ends inside channel '" + ch + "'");
        if (pixel_type != 2)
          return refuse(err, "channel '" + ch + "' of type " + (pixel_type == 1 ? "HALF" : pixel_type == 0 ? "UINT" : num(pixel_type)) +
                                 " (only FLOAT channels are read)");
        if (xs != 1 || ys != 1) return refuse(err, "channel '" + ch + "' with sampling " + num(xs) + " x " + num(ys) + " (only 1 x 1 is read)");
        int slot = -1;
        for (int k = 0; k < 14; k++)
          if (ch == kChannelNames[k]) slot = kChannelSource[k];
        if (slot >= 0)
          for (size_t k = 0; k < slots.size(); k++)
            if (slots[k] == slot) return refuse(err, "channel '" + ch + "' twice");
        if (slots.size() >= 1024) return refuse(err, "more than 1024 channels");
        slots.push_back(slot);
      }
    } else if (name == "compression") {
      if (type != "compression" || len != 1) return refuse(err, "attribute 'compression' of type '" + type + "' and " + num(len) + " bytes");
      if (bytes[v.at] != 0) return refuse(err, "compression " + num(bytes[v.at]) + " (only NONE = 0 is read)");
      have_compression = true;
    } else if (name == "dataWindow") {
      if (type != "box2i" || len != 16) return refuse(err, "attribute 'dataWindow' of type '" + type + "' and " + num(len) + " bytes");
      uint32_t b[4] = {0, 0, 0, 0};
      for (int k = 0; k < 4; k++) (void)v.u32(&b[k]);
      if (b[0] != 0 || b[1] != 0) return refuse(err, "a data window starting at (" + num((int32_t)b[0]) + ", " + num((int32_t)b[1]) + "), not (0, 0)");
      if ((int32_t)b[2] < 0 || (int32_t)b[3] < 0 || b[2] >= 16384 || b[3] >= 16384)
        return refuse(err, "a data window ending at (" + num((int32_t)b[2]) + ", " + num((int32_t)b[3]) + "), outside 0 .. 16383");
      width = (int64_t)b[2] + 1, height = (int64_t)b[3] + 1;
      have_window = true;
    } else if (name == "lineOrder") {
      if (type != "lineOrder" || len != 1) return refuse(err, "attribute 'lineOrder' of type '" + type + "' and " + num(len) + " bytes");
      if (bytes[v.at] != 0) return refuse(err, "line order " + num(bytes[v.at]) + " (only INCREASING_Y = 0 is read)");
    } else if (name == "tiles" || type == "tiledesc") {
      return refuse(err, "a 'tiles' attribute (only scanline files are read)");
    }  // (every other attribute is skipped)
  }
  if (!have_channels) return refuse(err, "no 'channels' attribute");
  if (!have_compression) return refuse(err, "no 'compression' attribute");
  if (!have_window) return refuse(err, "no 'dataWindow' attribute");
  bool present[14];
  memset(present, 0, sizeof(present));
  for (size_t k = 0; k < slots.size(); k++)
    if (slots[k] >= 0) present[slots[k]] = true;
  static const char* const rgb[3] = {"Color.R", "Color.G", "Color.B"};
  for (int k = 0; k < 3; k++)
    if (!present[k]) return refuse(err, std::string("no channel '") + rgb[k] + "'");

  // the line-offset table, then one block per line: y, the byte count, the channels in file order
  const uint64_t row_bytes = (uint64_t)width * slots.size() * 4, block = 8 + row_bytes;
  const uint64_t rest = size - c.at;
  if ((uint64_t)height * 8 > rest) return refuse(err, "truncated file: the line-offset table of " + num(height) + " lines runs past the end");
  if ((uint64_t)height * block > rest - (uint64_t)height * 8)
    return refuse(err, "truncated file: " + num(height) + " lines of " + num((long long)block) + " bytes need more than the " + num((long long)size) +
                           " bytes there are");
  const unsigned char* table = bytes + c.at;
  out->buffer.assign((size_t)width * (size_t)height * 14, 0.0f);
  for (int64_t y = 0; y < height; y++) {
    const uint64_t off = le64(table + y * 8);
    if (off > size || size - off < block)
      return refuse(err, "line " + num(y) + ": offset " + num((long long)off) + " with " + num((long long)block) + " bytes runs past the end");
    const unsigned char* line = bytes + off;
    if (le32(line) != (uint32_t)y) return refuse(err, "line " + num(y) + ": the block at its offset is line " + num((int32_t)le32(line)));
    if (le32(line + 4) != row_bytes)
      return refuse(err, "line " + num(y) + ": a block of " + num(le32(line + 4)) + " bytes, not width x channels x 4 = " + num((long long)row_bytes));
    float* row = out->buffer.data() + (size_t)y * (size_t)width * 14;
    for (size_t k = 0; k < slots.size(); k++) {
      if (slots[k] < 0) continue;
      const unsigned char* src = line + 8 + k * (size_t)width * 4;
      for (int64_t x = 0; x < width; x++) {
        const uint32_t u = le32(src + x * 4);
        memcpy(row + x * 14 + slots[k], &u, 4);
      }
    }
  }
  out->width = (int)width, out->height = (int)height;
  memcpy(out->present, present, sizeof(present));
  return true;
}

inline bool LoadFeatureEXR(const std::string& filename, FeatureImage* out, std::string* err) {
  FILE* f = fopen(filename.c_str(), "rb");
  if (!f) return detail::refuse(err, "Cannot read the file.");
  std::vector<unsigned char> bytes;
  unsigned char chunk[65536];
  size_t n;
  while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return detail::refuse(err, "Cannot read the file.");
  return DecodeFeatureEXR(bytes.data(), bytes.size(), out, err);
}

}  // namespace ptexr
#endif
