// npy.cpp — see npy.h
#include "npy.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

namespace phantom {

namespace {

[[noreturn]] void refuse(const std::string& name, const std::string& why) { throw std::runtime_error(name + ": " + why); }

// the header dict: a cursor over [p, end) that never moves past end
struct Cursor {
  const unsigned char* p;
  const unsigned char* end;
  const std::string& name;

  void skip_space() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool at(char c) {
    skip_space();
    return p < end && *p == static_cast<unsigned char>(c);
  }
  void expect(char c, const char* where) {
    if (!at(c)) refuse(name, std::string("malformed header dict: expected '") + c + "' " + where);
    ++p;
  }
  std::string quoted(const char* where) {
    skip_space();
    if (p >= end || (*p != '\'' && *p != '"')) refuse(name, std::string("malformed header dict: expected a string ") + where);
    const unsigned char q = *p++;
    std::string s;
    while (p < end && *p != q) s.push_back(static_cast<char>(*p++));
    if (p >= end) refuse(name, "malformed header dict: unterminated string");
    ++p;
    return s;
  }
  std::string word() {
    skip_space();
    std::string s;
    while (p < end && ((*p >= 'A' && *p <= 'Z') || (*p >= 'a' && *p <= 'z'))) s.push_back(static_cast<char>(*p++));
    return s;
  }
  // a tuple of non-negative integers: (), (3,), (3, 4)
  std::vector<size_t> tuple() {
    expect('(', "before the shape");
    std::vector<size_t> dims;
    while (!at(')')) {
      skip_space();
      if (p >= end || *p < '0' || *p > '9') refuse(name, "malformed header dict: the shape is not a tuple of integers");
      size_t v = 0;
      while (p < end && *p >= '0' && *p <= '9') {
        const size_t d = static_cast<size_t>(*p - '0');
        if (v > (std::numeric_limits<size_t>::max() - d) / 10) refuse(name, "a dimension overflows size_t");
        v = v * 10 + d;
        ++p;
      }
      dims.push_back(v);
      if (at(',')) ++p;
      else if (!at(')')) refuse(name, "malformed header dict: the shape is not a tuple of integers");
    }
    ++p;
    return dims;
  }
};

double read_le_f4(const unsigned char* b) {
  const uint32_t u = uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16 | uint32_t(b[3]) << 24;
  float f;
  static_assert(sizeof f == sizeof u, "IEEE single");
  std::memcpy(&f, &u, sizeof f);
  return static_cast<double>(f);
}

double read_le_f8(const unsigned char* b) {
  uint64_t u = 0;
  for (int i = 7; i >= 0; --i) u = u << 8 | b[i];
  double d;
  static_assert(sizeof d == sizeof u, "IEEE double");
  std::memcpy(&d, &u, sizeof d);
  return d;
}

void need_dims(const NpyArray& a, size_t dims, const std::string& path) {
  if (a.shape.size() != dims)
    refuse(path, "expected " + std::to_string(dims) + " dimensions, the file has " + std::to_string(a.shape.size()));
}

}  // namespace

NpyArray ParseNpy(const unsigned char* bytes, size_t size, const std::string& name) {
  static const unsigned char magic[6] = {0x93, 'N', 'U', 'M', 'P', 'Y'};
  if (size < 8 || std::memcmp(bytes, magic, 6) != 0) refuse(name, "not an .npy file (wrong magic)");
  const unsigned major = bytes[6], minor = bytes[7];
  if (!((major == 1 || major == 2) && minor == 0))
    refuse(name, "unsupported .npy version " + std::to_string(major) + "." + std::to_string(minor));
  const size_t len_bytes = major == 1 ? 2 : 4;
  if (size < 8 + len_bytes) refuse(name, "the header length runs past the end of the file");
  size_t header_len = 0;
  for (size_t i = 0; i < len_bytes; ++i) header_len |= size_t(bytes[8 + i]) << (8 * i);
  const size_t header_at = 8 + len_bytes;
  if (header_len > size - header_at) refuse(name, "the header length runs past the end of the file");

  Cursor c{bytes + header_at, bytes + header_at + header_len, name};
  bool have_descr = false, have_order = false, have_shape = false, fortran = false;
  std::string descr;
  std::vector<size_t> shape;
  c.expect('{', "at the start");
  while (!c.at('}')) {
    const std::string key = c.quoted("as a key");
    c.expect(':', "after a key");
    if (key == "descr") {
      if (!c.at('\'') && !c.at('"')) refuse(name, "unsupported dtype (a structured descr)");
      descr = c.quoted("as descr");
      have_descr = true;
    } else if (key == "fortran_order") {
      const std::string w = c.word();
      if (w != "True" && w != "False") refuse(name, "malformed header dict: fortran_order is neither True nor False");
      fortran = w == "True";
      have_order = true;
    } else if (key == "shape") {
      shape = c.tuple();
      have_shape = true;
    } else {
      refuse(name, "malformed header dict: unknown key '" + key + "'");
    }
    if (c.at(',')) ++c.p;
    else if (!c.at('}')) refuse(name, "malformed header dict: expected ',' or '}'");
  }
  if (!have_descr || !have_order || !have_shape)
    refuse(name, "the header dict lacks 'descr', 'fortran_order' or 'shape'");
  size_t item = 0;
  if (descr == "<f4") item = 4;
  else if (descr == "<f8") item = 8;
  else refuse(name, "unsupported dtype or byte order '" + descr + "' (only '<f4' and '<f8')");
  if (fortran) refuse(name, "Fortran-order arrays are not supported");
  if (shape.empty() || shape.size() > 4)
    refuse(name, "expected 1 to 4 dimensions, the file has " + std::to_string(shape.size()));
  size_t count = 1;
  for (size_t d : shape) {
    if (d == 0) refuse(name, "a dimension is 0");
    if (count > std::numeric_limits<size_t>::max() / d) refuse(name, "the shape's product overflows size_t");
    count *= d;
  }
  if (count > std::numeric_limits<size_t>::max() / item) refuse(name, "the shape's product overflows size_t");
  const size_t data_at = header_at + header_len, left = size - data_at;
  if (count * item > left) refuse(name, "truncated: the shape needs " + std::to_string(count * item) + " bytes of data, the file has " + std::to_string(left));
  if (count * item < left) refuse(name, "trailing bytes: the shape needs " + std::to_string(count * item) + " bytes of data, the file has " + std::to_string(left));

  NpyArray a;
  a.shape = std::move(shape);
  a.item_bytes = item;
  a.data.resize(count);
  const unsigned char* d = bytes + data_at;
  for (size_t i = 0; i < count; ++i) a.data[i] = item == 4 ? read_le_f4(d + 4 * i) : read_le_f8(d + 8 * i);
  return a;
}

NpyArray LoadNpy(const std::string& path) {
  std::unique_ptr<std::FILE, int (*)(std::FILE*)> f(std::fopen(path.c_str(), "rb"), &std::fclose);
  if (!f) refuse(path, "cannot open the file");
  std::vector<unsigned char> bytes;
  unsigned char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, f.get())) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
  if (std::ferror(f.get())) refuse(path, "read error");
  return ParseNpy(bytes.data(), bytes.size(), path);
}

NpyWeight4 LoadWeight4D(const std::string& path) {
  const NpyArray a = LoadNpy(path);
  need_dims(a, 4, path);
  const size_t O = a.shape[0], I = a.shape[1], H = a.shape[2], W = a.shape[3];
  NpyWeight4 w(H, std::vector<std::vector<std::vector<double>>>(W, std::vector<std::vector<double>>(I, std::vector<double>(O))));
  for (size_t o = 0; o < O; ++o)
    for (size_t i = 0; i < I; ++i)
      for (size_t h = 0; h < H; ++h)
        for (size_t x = 0; x < W; ++x) w[h][x][i][o] = a.data[((o * I + i) * H + h) * W + x];
  return w;
}

std::vector<std::vector<double>> LoadWeight2D(const std::string& path) {
  const NpyArray a = LoadNpy(path);
  need_dims(a, 2, path);
  std::vector<std::vector<double>> w(a.shape[0]);
  for (size_t r = 0; r < a.shape[0]; ++r) w[r].assign(a.data.begin() + r * a.shape[1], a.data.begin() + (r + 1) * a.shape[1]);
  return w;
}

std::vector<double> LoadWeight1D(const std::string& path) {
  NpyArray a = LoadNpy(path);
  need_dims(a, 1, path);
  return std::move(a.data);
}

NpyTensor3 LoadImage(const std::string& path, size_t index) {
  const NpyArray a = LoadNpy(path);
  need_dims(a, 4, path);
  const size_t C = a.shape[1], H = a.shape[2], W = a.shape[3];
  if (index >= a.shape[0])
    refuse(path, "image index " + std::to_string(index) + " is out of range (" + std::to_string(a.shape[0]) + " images)");
  if (H != W) refuse(path, "the images are not square");
  NpyTensor3 t(H, std::vector<std::vector<double>>(W, std::vector<double>(C)));
  for (size_t c = 0; c < C; ++c)
    for (size_t i = 0; i < H; ++i)
      for (size_t j = 0; j < W; ++j) t[i][j][c] = a.data[((index * C + c) * H + i) * W + j];
  return t;
}

}  // namespace phantom
