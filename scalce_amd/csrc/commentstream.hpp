// commentstream.hpp -- the comment stream of an archive made with --keep-comments (PREFIX_<m>.scalcec), host side only: no
// device call, no HIP header.  Layout: the 8 magic bytes, int32 0 (entry width 0: text entries -- .scalcel has 1 or 2, .scalceo
// 4), int32 C (the longest entry in bytes, without its terminator), int64 N, then N entries in archive order, each followed by
// '\n'.  An entry is what follows the name on the record's header line, from the first space inclusive to the newline
// exclusive: empty for a line without a space.  Header write and read with the text of every failure, and a cursor that hands
// out or passes over n entries by their newlines.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace scalce_host {

constexpr size_t COMMENT_HEADER_BYTES = 24;
constexpr uint32_t COMMENT_MAX_ENTRY = 65535;
static const uint8_t COMMENT_MAGIC[8] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'};

inline void comment_header_write(uint8_t out[COMMENT_HEADER_BYTES], uint32_t longest, uint64_t n) {
  const int32_t f[2] = {0, (int32_t)longest};
  memcpy(out, COMMENT_MAGIC, 8);
  memcpy(out + 8, f, 8);
  memcpy(out + 16, &n, 8);
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
  if (have < COMMENT_HEADER_BYTES) return comment_truncated();
  if (memcmp(h, COMMENT_MAGIC, 7)) return comment_not_a_stream();
  int32_t f[2];
  memcpy(f, h + 8, 8);
  if (f[0] != 0 || f[1] < 0 || f[1] > (int32_t)COMMENT_MAX_ENTRY) return comment_not_a_stream();
  int64_t v;
  memcpy(&v, h + 16, 8);
  if (v < 0 || v > 0xFFFFFFFFll) return comment_not_a_stream();
  *longest = (uint32_t)f[1];
  *n = (uint64_t)v;
  return nullptr;
}

// The entries behind the header, read through a callback of scalce_read_fn's contract: rd(user, dst, cap) stores any number of
// bytes up to cap and returns it, 0 at the end of the stream, < 0 on error.  take() appends the next n entries, each with its
// newline, to `out` (nullptr: they are passed over) and returns nullptr, or the text of what is wrong: a stream that ends
// inside an entry or before n entries, an entry longer than the header's C, a read that failed.
struct CommentCursor {
  typedef int64_t (*read_fn)(void *user, void *dst, uint64_t cap);
  read_fn rd = nullptr;
  void *user = nullptr;
  uint32_t longest = 0;   // the header's C
  uint64_t total = 0;     // the header's N
  uint64_t taken = 0;     // entries handed out or passed over so far
  uint64_t bytes = 0;     // ... and their bytes, newlines included
  std::vector<uint8_t> buf;
  size_t at = 0, have = 0;
  bool ended = false;
  uint64_t open_len = 0;  // bytes of the entry that is open across calls to fill()

  void start(read_fn r, void *u, size_t buffer_bytes = 1u << 16) {
    rd = r; user = u;
    buf.assign(buffer_bytes ? buffer_bytes : 1, 0);
    at = have = 0;
    taken = bytes = open_len = 0;
    ended = false;
  }
  // more bytes into the buffer; false at the stream's end or on a failed read (*failed)
  bool fill(bool *failed) {
    *failed = false;
    if (ended) return false;
    const int64_t k = rd(user, buf.data(), buf.size());
    if (k < 0) { *failed = true; ended = true; return false; }
    if (k == 0) { ended = true; return false; }
    at = 0;
    have = (size_t)k;
    return true;
  }
  // the header, through the same callback
  const char *read_header() {
    uint8_t h[COMMENT_HEADER_BYTES];
    size_t got = 0;
    while (got < COMMENT_HEADER_BYTES) {
      if (at == have) {
        bool failed;
        if (!fill(&failed)) return failed ? "comment stream: read failed" : comment_header_read(h, got, &longest, &total);
      }
      const size_t k = have - at < COMMENT_HEADER_BYTES - got ? have - at : COMMENT_HEADER_BYTES - got;
      memcpy(h + got, buf.data() + at, k);
      at += k;
      got += k;
    }
    return comment_header_read(h, got, &longest, &total);
  }
  const char *take(uint64_t n, std::vector<uint8_t> *out) {
    while (n) {
      if (at == have) {
        bool failed;
        if (!fill(&failed)) return failed ? "comment stream: read failed" : comment_truncated();
      }
      const uint8_t *p = buf.data() + at;
      const size_t room = have - at;
      const uint8_t *nl = static_cast<const uint8_t *>(memchr(p, '\n', room));
      const size_t k = nl ? (size_t)(nl - p) + 1 : room;  // bytes of this entry in the buffer, its newline included
      if (open_len + (nl ? k - 1 : k) > longest) return comment_entry_too_long();
      if (out) out->insert(out->end(), p, p + k);
      at += k;
      bytes += k;
      if (nl) { open_len = 0; taken++; n--; }
      else open_len += k;
    }
    return nullptr;
  }
  const char *skip(uint64_t n) { return take(n, nullptr); }
  // behind the archive's last record: nullptr when the stream holds exactly the entries the archive has records; else the
  // message in msg.  `records`: what the archive says it holds (the header's N is checked against it up front where known)
  const char *check_count(uint64_t records, char *msg, size_t cap) const {
    if (total == records) return nullptr;
    comment_count_message(msg, cap, total, records);
    return msg;
  }
};

}  // namespace scalce_host
