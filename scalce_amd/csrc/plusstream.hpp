// plusstream.hpp -- the plus-line stream of an archive made with --keep-plus (PREFIX_<m>.scalcep), host side only: no device
// call, no HIP header.  Layout: the 8 magic bytes, int32 0 (entry width 0: text entries, as in .scalcec), int32 P (the longest
// stored entry in bytes, without its terminator), int64 N, then N entries in archive order, each followed by '\n'.  P = 0: the
// file is its header, every record's third line was a bare '+'.  An entry is empty (bare '+'), the byte '=' (the line repeats
// the header line behind its '@') or '\'' followed by the line's bytes behind the '+'.  Header write and read with the text of
// every failure, the class of an entry, and a cursor that hands out or passes over n entries by their newlines.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace scalce_host {

constexpr size_t PLUS_HEADER_BYTES = 24;
constexpr uint32_t PLUS_MAX_ENTRY = 65535;
static const uint8_t PLUS_MAGIC[8] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'};
enum PlusClass { PLUS_BARE = 0, PLUS_REPEAT = 1, PLUS_LITERAL = 2, PLUS_MALFORMED = 3 };

inline void plus_header_write(uint8_t out[PLUS_HEADER_BYTES], uint32_t longest, uint64_t n) {
  const int32_t f[2] = {0, (int32_t)longest};
  memcpy(out, PLUS_MAGIC, 8);
  memcpy(out + 8, f, 8);
  memcpy(out + 16, &n, 8);
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
  if (have < PLUS_HEADER_BYTES) return plus_truncated();
  if (memcmp(h, PLUS_MAGIC, 7)) return plus_not_a_stream();
  int32_t f[2];
  memcpy(f, h + 8, 8);
  if (f[0] != 0 || f[1] < 0 || f[1] > (int32_t)PLUS_MAX_ENTRY) return plus_not_a_stream();
  int64_t v;
  memcpy(&v, h + 16, 8);
  if (v < 0 || v > 0xFFFFFFFFll) return plus_not_a_stream();
  *longest = (uint32_t)f[1];
  *n = (uint64_t)v;
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

// The entries behind the header, read through a callback of scalce_read_fn's contract: rd(user, dst, cap) stores any number of
// bytes up to cap and returns it, 0 at the end of the stream, < 0 on error.  take() appends the next n entries, each with its
// newline, to `out` (nullptr: they are passed over) and returns nullptr, or the text of what is wrong: a stream that ends
// inside an entry or before n entries, an entry longer than the header's P, a malformed entry, a read that failed.  With P = 0
// nothing is read: every entry is empty.
struct PlusCursor {
  typedef int64_t (*read_fn)(void *user, void *dst, uint64_t cap);
  read_fn rd = nullptr;
  void *user = nullptr;
  uint32_t longest = 0;   // the header's P
  uint64_t total = 0;     // the header's N
  uint64_t taken = 0;     // entries handed out or passed over so far
  uint64_t bytes = 0;     // ... and their bytes, newlines included
  uint64_t repeats = 0, literals = 0;
  std::vector<uint8_t> buf;
  size_t at = 0, have = 0;
  bool ended = false;
  uint64_t open_len = 0;  // bytes of the entry that is open across calls to fill()
  uint8_t open_class = 0; // ... and its first byte

  void start(read_fn r, void *u, size_t buffer_bytes = 1u << 16) {
    rd = r; user = u;
    buf.assign(buffer_bytes ? buffer_bytes : 1, 0);
    at = have = 0;
    taken = bytes = open_len = repeats = literals = 0;
    ended = false;
  }
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
  const char *read_header() {
    uint8_t h[PLUS_HEADER_BYTES];
    size_t got = 0;
    while (got < PLUS_HEADER_BYTES) {
      if (at == have) {
        bool failed;
        if (!fill(&failed)) return failed ? "plus-line stream: read failed" : plus_header_read(h, got, &longest, &total);
      }
      const size_t k = have - at < PLUS_HEADER_BYTES - got ? have - at : PLUS_HEADER_BYTES - got;
      memcpy(h + got, buf.data() + at, k);
      at += k;
      got += k;
    }
    return plus_header_read(h, got, &longest, &total);
  }
  const char *take(uint64_t n, std::vector<uint8_t> *out) {
    if (!longest) {  // the P = 0 form
      if (out) out->insert(out->end(), (size_t)n, (uint8_t)'\n');
      taken += n;
      return nullptr;
    }
    while (n) {
      if (at == have) {
        bool failed;
        if (!fill(&failed)) return failed ? "plus-line stream: read failed" : plus_truncated();
      }
      const uint8_t *p = buf.data() + at;
      const size_t room = have - at;
      const uint8_t *nl = static_cast<const uint8_t *>(memchr(p, '\n', room));
      const size_t k = nl ? (size_t)(nl - p) + 1 : room;  // bytes of this entry in the buffer, its newline included
      const size_t body = nl ? k - 1 : k;
      if (open_len + body > longest) return plus_entry_too_long();
      if (!open_len && body) open_class = p[0];
      if (out) out->insert(out->end(), p, p + k);
      at += k;
      bytes += k;
      if (nl) {
        const uint64_t len = open_len + body;
        if (len) {
          if (open_class == '=' && len == 1) repeats++;
          else if (open_class == '\'' && len > 1) literals++;
          else return plus_malformed();
        }
        open_len = 0; taken++; n--;
      } else open_len += k;
    }
    return nullptr;
  }
  const char *skip(uint64_t n) { return take(n, nullptr); }
  const char *check_count(uint64_t records, char *msg, size_t cap) const {
    if (total == records) return nullptr;
    plus_count_message(msg, cap, total, records);
    return msg;
  }
};

}  // namespace scalce_host
