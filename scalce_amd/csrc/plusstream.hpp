// plusstream.hpp -- the plus-line stream of an archive made with --keep-plus (PREFIX_<m>.scalcep), host side only: no device
// call, no HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 0 (entry width 0: text entries, as in .scalcec),
// int32 P (the longest stored entry in bytes, without its terminator), int64 N, then N entries in archive order, each followed
// by '\n'.  P = 0: the file is its header, every record's third line was a bare '+'.  An entry is empty (bare '+'), the byte
// '=' (the line repeats the header line behind its '@') or '\'' followed by the line's bytes behind the '+'.  Header write and
// read with the text of every failure, and the class of an entry; the entries are walked by their newlines in
// archive_walk.hpp.
#pragma once
#include <cstdio>

#include "sidestream.hpp"

namespace scalce_host {

constexpr size_t PLUS_HEADER_BYTES = side_header_bytes(1);
constexpr uint32_t PLUS_MAX_ENTRY = 65535;
enum PlusClass { PLUS_BARE = 0, PLUS_REPEAT = 1, PLUS_LITERAL = 2, PLUS_MALFORMED = 3 };

inline void plus_header_write(uint8_t out[PLUS_HEADER_BYTES], uint32_t longest, uint64_t n) {
  side_header_write(out, 1, SideHeader{0, (int32_t)longest, {(int64_t)n}});
}
inline const char *plus_truncated() { return "truncated plus-line stream"; }
inline const char *plus_not_a_stream() { return "is not a scalce plus-line stream"; }
inline const char *plus_entry_too_long() { return "plus-line stream: an entry is longer than its header says"; }
inline const char *plus_malformed() { return "plus-line stream: malformed entry"; }
inline int plus_count_message(char *out, size_t cap, uint64_t entries, uint64_t records) {
  return snprintf(out, cap, "plus-line stream holds %llu entries, the archive %llu records", (unsigned long long)entries,
                  (unsigned long long)records);
}
// nullptr: a header this build reads (*longest, *n filled in); else what is wrong with it
inline const char *plus_header_read(const uint8_t *h, size_t have, uint32_t *longest, uint64_t *n) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, have, 1, &f);
  if (st == SIDE_SHORT) return plus_truncated();
  if (st == SIDE_NOT_OURS || f.width != 0 || f.param < 0 || f.param > (int32_t)PLUS_MAX_ENTRY || f.count[0] < 0 || f.count[0] > 0xFFFFFFFFll)
    return plus_not_a_stream();
  *longest = (uint32_t)f.param;
  *n = (uint64_t)f.count[0];
  return nullptr;
}
// what an entry of `len` bytes (its newline not counted) is
inline PlusClass plus_class(const uint8_t *e, size_t len) {
  if (!len) return PLUS_BARE;
  if (e[0] == '=') return len == 1 ? PLUS_REPEAT : PLUS_MALFORMED;
  if (e[0] == '\'') return len > 1 ? PLUS_LITERAL : PLUS_MALFORMED;  // (an empty literal would be the bare line)
  return PLUS_MALFORMED;
}
// bytes a record's text grows by when its entry goes back: header_bytes = the header line behind its '@'
inline uint64_t plus_growth(PlusClass c, size_t len, uint64_t header_bytes) {
  return c == PLUS_REPEAT ? header_bytes : c == PLUS_LITERAL ? (uint64_t)len - 1 : 0;
}

}  // namespace scalce_host
