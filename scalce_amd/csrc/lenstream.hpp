// lenstream.hpp -- the length stream of a variable-length archive (PREFIX_<m>.scalcel), host side only: no device call, no
// HIP header.  Layout: the 8 magic bytes, int32 entry width (1 if L <= 255, else 2), int32 L, then one little-endian entry
// per record in archive order holding L - length.  The writer (cli.cpp) and the reader (stream_decode.cpp) share it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace scalce_host {

constexpr size_t LEN_HEADER_BYTES = 16;
static const uint8_t LEN_MAGIC[8] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'};

inline int len_entry_width(int L) { return L <= 255 ? 1 : 2; }

inline void len_header_write(uint8_t out[LEN_HEADER_BYTES], int L) {
  const int32_t f[2] = {len_entry_width(L), L};
  memcpy(out, LEN_MAGIC, 8);
  memcpy(out + 8, f, 8);
}
// nullptr: a header this build reads (*width, *L filled in); else what is wrong with it
inline const char *len_header_read(const uint8_t *h, size_t n, int *width, int *L) {
  if (n < LEN_HEADER_BYTES) return "truncated length stream";
  if (memcmp(h, LEN_MAGIC, 7)) return "is not a scalce length stream";
  int32_t f[2];
  memcpy(f, h + 8, 8);
  if (f[1] <= 0 || f[1] > 65535) return "length stream: read length out of range";
  if (f[0] != len_entry_width(f[1])) return "length stream: entry width does not fit its read length";
  *width = f[0];
  *L = f[1];
  return nullptr;
}
// n entries of L - length -> n * width bytes
inline void len_entries_write(const uint16_t *pad, size_t n, int width, uint8_t *out) {
  if (width == 1) { for (size_t i = 0; i < n; i++) out[i] = (uint8_t)pad[i]; return; }
  for (size_t i = 0; i < n; i++) { out[2 * i] = (uint8_t)(pad[i] & 255); out[2 * i + 1] = (uint8_t)(pad[i] >> 8); }
}
// the sum of n entries, or ~0 when one of them is above L (no read is shorter than nothing)
inline uint64_t len_entries_sum(const uint8_t *in, size_t n, int width, int L) {
  uint64_t sum = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t v = width == 1 ? in[i] : (uint32_t)in[2 * i] | ((uint32_t)in[2 * i + 1] << 8);
    if (v > (uint32_t)L) return ~0ull;
    sum += v;
  }
  return sum;
}

}  // namespace scalce_host
