// orderstream.hpp -- the order stream of an archive made with --keep-order (PREFIX_1.scalceo), host side only: no device call,
// no HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 entry width (4), int32 0, int64 N, then N little-endian u32: entry k is the
// input index of the k-th record (pair) of the archive.  The writer (cli.cpp) and the reader (stream_decode.cpp) share it, and
// the table that says where each window's share of each stripe lies in the spill of the restore, with the spill's record word
// and the spill file itself.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sidestream.hpp"

namespace scalce_host {

constexpr size_t ORDER_HEADER_BYTES = side_header_bytes(1);
constexpr int ORDER_ENTRY_WIDTH = 4;
constexpr uint64_t ORDER_MAX_STRIPES = 65536;

inline void order_header_write(uint8_t out[ORDER_HEADER_BYTES], uint64_t n) {
  side_header_write(out, 1, SideHeader{ORDER_ENTRY_WIDTH, 0, {(int64_t)n}});
}
// nullptr: a header this build reads (*n filled in); else what is wrong with it
inline const char *order_header_read(const uint8_t *h, size_t have, uint64_t *n) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, have, 1, &f);
  if (st == SIDE_SHORT) return "truncated order stream";
  if (st == SIDE_NOT_OURS || f.width != ORDER_ENTRY_WIDTH || f.param != 0 || f.count[0] < 0 || f.count[0] > 0xFFFFFFFFll)
    return "is not a scalce order stream";
  *n = (uint64_t)f.count[0];
  return nullptr;
}
// the other messages of the stream; `entries` against the `records` the archive holds
inline const char *order_not_permutation() { return "order stream is not a permutation of the records"; }
inline int order_count_message(char *out, size_t cap, uint64_t entries, uint64_t records) {
  return snprintf(out, cap, "order stream holds %llu entries, the archive %llu records", (unsigned long long)entries,
                  (unsigned long long)records);
}
// host-side check of n entries: false when one of them is >= total (the device checks the same; this one serves callers
// that hold the entries anyway)
inline bool order_entries_in_range(const uint32_t *e, size_t n, uint64_t total) {
  for (size_t i = 0; i < n; i++)
    if ((uint64_t)e[i] >= total) return false;
  return true;
}

// R records per stripe and S stripes for N records, from the window and the bound of a record's text: R = window /
// max_record_bytes (at least 1), raised where needed so that S = ceil(N / R) <= ORDER_MAX_STRIPES
inline void order_plan(uint64_t total, uint64_t window, uint64_t max_record_bytes, uint64_t out[2]) {
  uint64_t R = max_record_bytes ? window / max_record_bytes : window;
  if (R < 1) R = 1;
  uint64_t S = (total + R - 1) / R;
  if (S > ORDER_MAX_STRIPES) {
    R = (total + ORDER_MAX_STRIPES - 1) / ORDER_MAX_STRIPES;
    S = (total + R - 1) / R;
  }
  out[0] = R;
  out[1] = S;
}

// what the spill keeps per record beside its text: the record's entry of the order stream and the bytes of its text
inline uint64_t record_word(uint32_t entry, uint64_t size) { return (uint64_t)entry | size << 32; }
inline uint32_t record_entry(uint64_t word) { return (uint32_t)word; }
inline uint64_t record_size(uint64_t word) { return word >> 32; }

// Where each window's share of each stripe lies in the spill.  A window's records are appended grouped by stripe, so its
// share of stripe s follows its share of stripe s - 1: the table keeps, per window, where its records begin in the text and
// in the record words, and its non-empty shares; stripes are then taken in rising order and every window keeps a cursor.
struct StripeTable {
  struct Share { uint32_t stripe, records; uint64_t bytes; };
  struct Piece { uint64_t text_at, bytes, record_at, records; };  // one pread of text, one of record words
  struct Win { uint64_t text_at, record_at; size_t first, n, cur; };
  uint64_t S = 0, next_stripe = 0;
  uint64_t text_bytes = 0, records = 0;  // appended so far
  std::vector<Share> shares;
  std::vector<Win> wins;
  void reset(uint64_t stripes) { *this = StripeTable(); S = stripes; }
  // a window of n records: counts[s] of them in stripe s (S entries), off[k] where the k-th of them begins in the window's
  // grouped text (n + 1 entries).  false: the counts do not add up to n
  bool add_window(const uint32_t *counts, const uint64_t *off, uint64_t n) {
    Win w{text_bytes, records, shares.size(), 0, 0};
    uint64_t at = 0;
    for (uint64_t s = 0; s < S; s++) {
      const uint64_t c = counts[s];
      if (!c) continue;
      if (at + c > n) { shares.resize(w.first); return false; }
      shares.push_back(Share{(uint32_t)s, (uint32_t)c, off[at + c] - off[at]});
      at += c;
    }
    if (at != n) { shares.resize(w.first); return false; }
    w.n = shares.size() - w.first;
    wins.push_back(w);
    text_bytes += off[n] - off[0];
    records += n;
    return true;
  }
  // the pieces of the next stripe, in window order (stripes are asked for in order 0, 1, ..); returns its records
  uint64_t take_stripe(std::vector<Piece> &out, uint64_t *bytes) {
    out.clear();
    uint64_t rec = 0, by = 0;
    const uint64_t s = next_stripe++;
    for (Win &w : wins) {
      if (w.cur == w.n || shares[w.first + w.cur].stripe != s) continue;
      const Share &sh = shares[w.first + w.cur++];
      out.push_back(Piece{w.text_at, sh.bytes, w.record_at, sh.records});
      w.text_at += sh.bytes;
      w.record_at += sh.records;
      rec += sh.records;
      by += sh.bytes;
    }
    if (bytes) *bytes = by;
    return rec;
  }
};

// One file of the spill: made once with mkstemp and unlinked at once -- nothing stays behind whatever happens --, emptied
// when a further mate pass begins, closed when it goes.  A false return leaves errno for the caller's message.
struct SpillFile {
  int fd = -1;
  uint64_t piece = 1u << 30;  // the most one call moves (tools/orderstream_check.cpp lowers it)
  SpillFile() = default;
  SpillFile(const SpillFile &) = delete;
  SpillFile &operator=(const SpillFile &) = delete;
  ~SpillFile() { if (fd >= 0) ::close(fd); }
  // *what: the verb of the step that failed ("make", "empty")
  bool reset(const std::string &dir, const char **what) {
    if (fd >= 0) { *what = "empty"; return ftruncate(fd, 0) == 0; }
    *what = "make";
    std::string path = dir + "/scalce_order_XXXXXX";
    fd = mkstemp(&path[0]);
    if (fd >= 0) unlink(path.c_str());
    return fd >= 0;
  }
  // n bytes at `at`, written from p or read into it: interrupted calls are repeated, a write that takes nothing is a full
  // disk (ENOSPC), a read that gives nothing lies behind the file's end (EIO)
  bool transfer(bool write, void *p, uint64_t n, uint64_t at) {
    uint8_t *b = static_cast<uint8_t *>(p);
    while (n) {
      const size_t want = (size_t)std::min(n, piece);
      const ssize_t k = write ? ::pwrite(fd, b, want, (off_t)at) : ::pread(fd, b, want, (off_t)at);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) { if (!k) errno = write ? ENOSPC : EIO; return false; }
      b += k; n -= (uint64_t)k; at += (uint64_t)k;
    }
    return true;
  }
};

}  // namespace scalce_host
