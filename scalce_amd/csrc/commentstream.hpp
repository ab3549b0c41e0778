// commentstream.hpp -- the comment stream of an archive made with --keep-comments (PREFIX_<m>.scalcec), host side only: no
// device call, no HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 0 (entry width 0: text entries -- .scalcel has
// 1 or 2, .scalceo 4), int32 C (the longest entry in bytes, without its terminator), int64 N, then N entries in archive order,
// each followed by '\n'.  An entry is what follows the name on the record's header line, from the first space inclusive to the
// newline exclusive: empty for a line without a space.  Header write and read with the text of every failure; the entries
// are walked by their newlines in archive_walk.hpp.
#pragma once
#include <cstdio>

#include "sidestream.hpp"

namespace scalce_host {

constexpr size_t COMMENT_HEADER_BYTES = side_header_bytes(1);
constexpr uint32_t COMMENT_MAX_ENTRY = 65535;

inline void comment_header_write(uint8_t out[COMMENT_HEADER_BYTES], uint32_t longest, uint64_t n) {
  side_header_write(out, 1, SideHeader{0, (int32_t)longest, {(int64_t)n}});
}
inline const char *comment_truncated() { return "truncated comment stream"; }
inline const char *comment_not_a_stream() { return "is not a scalce comment stream"; }
inline const char *comment_entry_too_long() { return "comment stream: an entry is longer than its header says"; }
inline int comment_count_message(char *out, size_t cap, uint64_t entries, uint64_t records) {
  return snprintf(out, cap, "comment stream holds %llu entries, the archive %llu records", (unsigned long long)entries,
                  (unsigned long long)records);
}
// nullptr: a header this build reads (*longest, *n filled in); else what is wrong with it
inline const char *comment_header_read(const uint8_t *h, size_t have, uint32_t *longest, uint64_t *n) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, have, 1, &f);
  if (st == SIDE_SHORT) return comment_truncated();
  if (st == SIDE_NOT_OURS || f.width != 0 || f.param < 0 || f.param > (int32_t)COMMENT_MAX_ENTRY || f.count[0] < 0 || f.count[0] > 0xFFFFFFFFll)
    return comment_not_a_stream();
  *longest = (uint32_t)f.param;
  *n = (uint64_t)f.count[0];
  return nullptr;
}

}  // namespace scalce_host
