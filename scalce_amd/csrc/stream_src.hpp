// stream_src.hpp -- one stream of an archive behind its read callback, as the decompress host (archive_walk.hpp) walks it.
// Host side only: callbacks and a std::vector, no device call, no HIP header, so that its arithmetic can be run on its own
// (tools/src_check.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/scalce_hip.h"

namespace scalce_host {
typedef uint8_t u8;
typedef uint64_t u64;
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one stream of the archive behind its read callback: a look-ahead buffer for the parts the host walks (headers, names,
// frame sizes), bulk reads straight into the caller's pinned memory for the rest
struct Src {
  scalce_read_fn rd = nullptr;
  scalce_skip_fn skp = nullptr;
  void *user = nullptr;
  std::vector<u8> buf;
  size_t pos = 0, end = 0;
  bool eof = false, bad = false;
  double *wait = nullptr;
  u64 *delivered = nullptr, *skipped = nullptr;
  void open(scalce_read_fn f, scalce_skip_fn sk, void *u, double *w, u64 *del, u64 *skd) {
    rd = f; skp = f ? sk : nullptr; user = u; wait = w; delivered = del; skipped = skd;
    buf.resize(SCALCE_UNPACK_LOOKAHEAD_BYTES);
  }
  size_t avail() const { return end - pos; }
  const u8 *ptr() const { return buf.data() + pos; }
  void skip(size_t n) { pos += n; }
  int64_t pull(void *dst, u64 cap) {
    if (!rd) { eof = true; return 0; }
    const double t0 = now_s();
    const int64_t k = rd(user, dst, cap);
    *wait += now_s() - t0;
    if (k < 0) bad = true;
    if (k == 0) eof = true;
    if (k > 0) *delivered += (u64)k;
    return k;
  }
  // false: the stream ends (or fails) before n bytes.  `look`: how far a refill may read ahead of the n bytes asked for --
  // the whole buffer for a stream that is read from end to end; less in front of bytes that are about to be passed over
  bool need(size_t n, size_t look = ~(size_t)0) { return end - pos >= n ? true : fill(n, look); }
  bool fill(size_t n, size_t look) {
    if (pos) { memmove(buf.data(), buf.data() + pos, end - pos); end -= pos; pos = 0; }
    if (buf.size() < n) buf.resize(n);
    while (end < n && !eof && !bad) {
      const int64_t k = pull(buf.data() + end, std::min(buf.size() - end, n - end + std::min(look, buf.size())));
      if (k > 0) end += (size_t)k;
    }
    return end >= n;
  }
  // the next little-endian T (a header field, a size word; the hosts are little-endian), or false: the stream ends, or
  // fails, before it -- nothing is taken then
  template <typename T> bool get(T &v, size_t look = ~(size_t)0) {
    if (!need(sizeof(T), look)) return false;
    memcpy(&v, ptr(), sizeof(T));
    skip(sizeof(T));
    return true;
  }
  // passes over n bytes: what the look-ahead buffer holds first, then the caller's skip, or -- without one -- reads that are
  // dropped; returns the bytes passed over (< n: the stream ends there, or has failed)
  u64 pass(u64 n) {
    u64 got = std::min<u64>(n, avail());
    pos += got;
    if (got < n && skp && !eof && !bad) {
      const double t0 = now_s();
      const int64_t k = skp(user, n - got);
      *wait += now_s() - t0;
      if (k < 0 || (u64)k > n - got) bad = true;
      else { got += (u64)k; *skipped += (u64)k; if (got < n) eof = true; }
      return got;
    }
    while (got < n && !eof && !bad) {
      pos = end = 0;
      const int64_t k = pull(buf.data(), std::min<u64>(buf.size(), n - got));
      if (k > 0) got += (u64)k;
    }
    return got;
  }
  // n bytes into dst: what the buffer holds first, then the callback directly; returns the bytes delivered (< n: the end)
  u64 read_into(u8 *dst, u64 n) {
    u64 got = std::min<u64>(n, avail());
    memcpy(dst, ptr(), got);
    pos += got;
    while (got < n && !eof && !bad) {
      const int64_t k = pull(dst + got, n - got);
      if (k > 0) got += (u64)k;
    }
    return got;
  }
};

}  // namespace scalce_host
