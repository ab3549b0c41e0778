// exceptionstream.hpp -- the exception stream of an archive made with --keep-bases (PREFIX_<m>.scalcex), host side only: no
// device call, no HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 8 (entry width), int32 L, int64 N (records), int64 X (entries),
// then X little-endian u64, strictly ascending by record and position (one entry per place): bits 0-7 the letter, 8-15 the quality character, 16-27 the position,
// 28-63 the record's index in archive order.  Header write and read with the text of every failure, and a cursor that hands
// out the entries of records [r0, r1) over a read callback: it passes over the entries in front of r0 and takes none behind
// r1.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sidestream.hpp"

namespace scalce_host {

constexpr size_t EXCEPTION_HEADER_BYTES = side_header_bytes(2);
constexpr int EXCEPTION_ENTRY_WIDTH = 8;
constexpr int EXCEPTION_POS_BITS = 12, EXCEPTION_REC_SHIFT = 28;
constexpr uint64_t EXCEPTION_MAX_RECORDS = 1ull << 36;

inline uint64_t exception_entry(uint64_t record, uint32_t pos, uint8_t letter, uint8_t quality) {
  return (uint64_t)letter | (uint64_t)quality << 8 | (uint64_t)pos << 16 | record << EXCEPTION_REC_SHIFT;
}
inline uint64_t exception_record(uint64_t e) { return e >> EXCEPTION_REC_SHIFT; }
inline uint32_t exception_pos(uint64_t e) { return (uint32_t)(e >> 16) & ((1u << EXCEPTION_POS_BITS) - 1u); }

inline void exception_header_write(uint8_t out[EXCEPTION_HEADER_BYTES], uint32_t read_len, uint64_t records, uint64_t entries) {
  side_header_write(out, 2, SideHeader{EXCEPTION_ENTRY_WIDTH, (int32_t)read_len, {(int64_t)records, (int64_t)entries}});
}
inline const char *exception_truncated() { return "truncated exception stream"; }
inline const char *exception_not_a_stream() { return "is not a scalce exception stream"; }
inline const char *exception_not_ascending() { return "exception stream: entries are not in ascending order"; }
inline const char *exception_outside() { return "exception stream: an entry lies outside its record"; }
inline const char *exception_read_failed() { return "exception stream: read failed"; }
inline int exception_count_message(char *out, size_t cap, uint64_t records, uint64_t archive) {
  return snprintf(out, cap, "exception stream holds %llu records, the archive %llu", (unsigned long long)records, (unsigned long long)archive);
}
inline int exception_length_message(char *out, size_t cap, uint32_t read_len, uint32_t archive) {
  return snprintf(out, cap, "exception stream is for reads of %u bases, the archive's have %u", read_len, archive);
}
// nullptr: a header this build reads (*read_len, *records, *entries filled in); else what is wrong with it
inline const char *exception_header_read(const uint8_t *h, size_t have, uint32_t *read_len, uint64_t *records, uint64_t *entries) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, have, 2, &f);
  if (st == SIDE_SHORT) return exception_truncated();
  if (st == SIDE_NOT_OURS || f.width != EXCEPTION_ENTRY_WIDTH || f.param <= 0 || f.param >= (1 << EXCEPTION_POS_BITS)) return exception_not_a_stream();
  const int64_t n = f.count[0], x = f.count[1];
  if (n < 0 || (uint64_t)n >= EXCEPTION_MAX_RECORDS || x < 0) return exception_not_a_stream();
  *read_len = (uint32_t)f.param;
  *records = (uint64_t)n;
  *entries = (uint64_t)x;
  return nullptr;
}

// The entries behind the header, read through a callback of scalce_read_fn's contract: rd(user, dst, cap) stores any number of
// bytes up to cap and returns it, 0 at the end of the stream, < 0 on error.  take(r0, r1, out) passes over the entries of
// records in front of r0, appends those of records [r0, r1) to `out` and leaves the first entry of a record at or behind r1
// for the next call; calls come with rising ranges.  It returns nullptr, or the text of what is wrong: a stream that ends
// before its X entries, entries that do not ascend, an entry whose record is not below N or whose position is not below L, a
// read that failed.
struct ExceptionCursor {
  typedef int64_t (*read_fn)(void *user, void *dst, uint64_t cap);
  read_fn rd = nullptr;
  void *user = nullptr;
  uint32_t read_len = 0;             // the header's L
  uint64_t records = 0, total = 0;   // the header's N and X
  uint64_t taken = 0;                // entries handed out or passed over so far
  uint64_t last = 0;                 // the last of them
  uint64_t pending = 0;              // an entry read and checked, not yet taken
  bool has_pending = false;
  std::vector<uint8_t> buf;
  size_t at = 0, have = 0;
  bool ended = false;

  void start(read_fn r, void *u, size_t buffer_bytes = 1u << 16) {
    rd = r; user = u;
    buf.assign(buffer_bytes ? buffer_bytes : 1, 0);
    at = have = 0;
    taken = last = pending = 0;
    has_pending = ended = false;
  }
  // n bytes into dst; *got = how many the stream still had.  false: a read failed
  bool fetch(uint8_t *dst, size_t n, size_t *got) {
    *got = 0;
    while (*got < n) {
      if (at == have) {
        if (ended) return true;
        const int64_t k = rd(user, buf.data(), buf.size());
        if (k < 0) { ended = true; return false; }
        if (k == 0) { ended = true; return true; }
        at = 0;
        have = (size_t)k;
      }
      const size_t k = have - at < n - *got ? have - at : n - *got;
      memcpy(dst + *got, buf.data() + at, k);
      at += k;
      *got += k;
    }
    return true;
  }
  const char *read_header() {
    uint8_t h[EXCEPTION_HEADER_BYTES];
    size_t got = 0;
    if (!fetch(h, sizeof h, &got)) return exception_read_failed();
    return exception_header_read(h, got, &read_len, &records, &total);
  }
  // the next entry, checked, into `pending`; *end: the stream's X entries are through
  const char *peek(bool *end) {
    *end = false;
    if (has_pending) return nullptr;
    if (taken == total) { *end = true; return nullptr; }
    uint8_t b[8];
    size_t got = 0;
    if (!fetch(b, 8, &got)) return exception_read_failed();
    if (got < 8) return exception_truncated();
    uint64_t e;
    memcpy(&e, b, 8);
    if (taken && (e >> 16) <= (last >> 16)) return exception_not_ascending();  // (record and position: one entry per place)
    if (exception_record(e) >= records || exception_pos(e) >= read_len) return exception_outside();
    pending = e;
    has_pending = true;
    return nullptr;
  }
  const char *take(uint64_t r0, uint64_t r1, std::vector<uint64_t> *out) {
    for (;;) {
      bool end;
      if (const char *why = peek(&end)) return why;
      if (end || exception_record(pending) >= r1) return nullptr;
      if (out && exception_record(pending) >= r0) out->push_back(pending);
      last = pending;
      has_pending = false;
      taken++;
    }
  }
};

}  // namespace scalce_host
