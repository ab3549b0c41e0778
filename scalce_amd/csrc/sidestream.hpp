// sidestream.hpp -- the header that the side files of an archive share (.scalcel, .scalceo, .scalcec, .scalcex, .scalcep,
// .scalced), host side only: no device call, no HIP header, nothing of the library.  Layout: the 8 magic bytes, int32 entry
// width, int32 a parameter of the stream's own, then zero, one or two int64 counts, all little-endian.  One writer and one
// reader of these fields; what the values may be, and the text of every failure, is each stream's own business
// (lenstream.hpp, orderstream.hpp, commentstream.hpp, exceptionstream.hpp, plusstream.hpp, digeststream.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace scalce_host {

// what every file of an archive begins with, the reference's three streams and ours
static const uint8_t ARCHIVE_MAGIC[8] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'};
constexpr size_t side_header_bytes(int counts) { return 16 + 8 * (size_t)counts; }

struct SideHeader {
  int32_t width = 0, param = 0;
  int64_t count[2] = {0, 0};
};
enum SideHeaderState { SIDE_OK = 0, SIDE_SHORT, SIDE_NOT_OURS };  // read; fewer bytes than the header; not our magic

// side_header_bytes(counts) bytes into out
inline void side_header_write(uint8_t *out, int counts, const SideHeader &h) {
  const int32_t f[2] = {h.width, h.param};
  memcpy(out, ARCHIVE_MAGIC, 8);
  memcpy(out + 8, f, 8);
  memcpy(out + 16, h.count, 8 * (size_t)counts);
}
// `have` bytes at h.  Seven bytes of the magic are compared, as the walk compares those of the archive's own three streams
inline SideHeaderState side_header_read(const uint8_t *h, size_t have, int counts, SideHeader *out) {
  if (have < side_header_bytes(counts)) return SIDE_SHORT;
  if (memcmp(h, ARCHIVE_MAGIC, 7)) return SIDE_NOT_OURS;
  int32_t f[2];
  memcpy(f, h + 8, 8);
  out->width = f[0];
  out->param = f[1];
  memcpy(out->count, h + 16, 8 * (size_t)counts);
  return SIDE_OK;
}

}  // namespace scalce_host
