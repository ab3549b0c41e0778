// lenstream.hpp -- the length stream of a variable-length archive (PREFIX_<m>.scalcel), host side only: no device call, no
// HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 entry width (1 if L <= 255, else 2), int32 L, then one
// little-endian entry per record in archive order holding L - length.  The writer (cli.cpp) and the reader (stream_decode.cpp)
// share it.
#pragma once
#include "sidestream.hpp"

namespace scalce_host {

constexpr size_t LEN_HEADER_BYTES = side_header_bytes(0);

inline int len_entry_width(int L) { return L <= 255 ? 1 : 2; }

inline void len_header_write(uint8_t out[LEN_HEADER_BYTES], int L) {
  side_header_write(out, 0, SideHeader{len_entry_width(L), L});
}
// nullptr: a header this build reads (*width, *L filled in); else what is wrong with it
inline const char *len_header_read(const uint8_t *h, size_t n, int *width, int *L) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, n, 0, &f);
  if (st == SIDE_SHORT) return "truncated length stream";
  if (st == SIDE_NOT_OURS) return "is not a scalce length stream";
  if (f.param <= 0 || f.param > 65535) return "length stream: read length out of range";
  if (f.width != len_entry_width(f.param)) return "length stream: entry width does not fit its read length";
  *width = f.width;
  *L = f.param;
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
