// src_check.cpp -- the stream cursor of the decompress host (scalce_amd/csrc/stream_src.hpp: need / fill / pass / read_into
// over a read and a skip callback) on its own: a program for AddressSanitizer, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/src_check.cpp -o /tmp/src_check && /tmp/src_check
// The stream is a byte string whose bytes tell their position, so bytes that arrive in the wrong order are seen; every
// destination is a heap block of exactly the size the call may touch, so a byte too far is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../scalce_amd/csrc/stream_src.hpp"

using scalce_host::Src;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static const size_t TOTAL = 5000;
static uint8_t byte_at(size_t i) { return (uint8_t)(i * 131 + (i >> 8) * 17 + 7); }

enum Read { ONE_BYTE, ODD_PIECES, ERROR_AT_K, ENDS_EARLY };
enum Skip { NO_SKIP, EXACT, SHORT, TOO_MUCH };

struct Feed {  // the stream behind the callbacks
  Read rd;
  Skip sk;
  size_t at = 0, limit = TOTAL;  // bytes handed out or skipped so far; where the stream ends
  int calls = 0, error_call = -1;
  static int64_t read_cb(void *user, void *dst, uint64_t cap) {
    Feed &f = *static_cast<Feed *>(user);
    static const size_t odd[5] = {3, 7, 1, 13, 5};
    CHECK(cap > 0);
    if (f.calls++ == f.error_call) return -1;
    size_t k = f.rd == ONE_BYTE ? 1 : odd[f.calls % 5];
    k = std::min<size_t>(std::min<size_t>(k, cap), f.limit - f.at);
    std::unique_ptr<uint8_t[]> piece(new uint8_t[k ? k : 1]);  // (what the callback writes is all it may write)
    for (size_t i = 0; i < k; i++) piece[i] = byte_at(f.at + i);
    memcpy(dst, piece.get(), k);
    f.at += k;
    return (int64_t)k;
  }
  static int64_t skip_cb(void *user, uint64_t n) {
    Feed &f = *static_cast<Feed *>(user);
    if (f.sk == TOO_MUCH) return (int64_t)n + 1;
    size_t k = std::min<size_t>(n, f.limit - f.at);
    if (f.sk == SHORT) k /= 2;  // fewer than asked: the stream ends there
    f.at += k;
    return (int64_t)k;
  }
};

static void drive(Read rd, Skip sk, size_t bufsize, unsigned seed) {
  Feed f{rd, sk};
  if (rd == ERROR_AT_K) f.error_call = 40 + (int)(seed % 7);
  if (rd == ENDS_EARLY) f.limit = TOTAL / 2 + seed % 11;
  double wait = 0;
  uint64_t delivered = 0, skipped = 0;
  Src s;
  s.open(Feed::read_cb, sk == NO_SKIP ? nullptr : Feed::skip_cb, &f, &wait, &delivered, &skipped);
  CHECK(s.buf.size() == SCALCE_UNPACK_LOOKAHEAD_BYTES);
  if (bufsize) { s.buf.resize(bufsize); s.buf.shrink_to_fit(); }  // a small buffer: refills, moves and growth all happen
  size_t P = 0;         // bytes the caller has consumed
  bool ended = false;   // a call has come back short: the stream has ended or failed, nothing more may arrive
  auto held_is_right = [&]() { for (size_t i = 0; i < s.avail(); i++) CHECK(s.ptr()[i] == byte_at(P + i)); };
  auto counters = [&]() { CHECK(delivered + skipped == f.at && P + s.avail() == f.at); };
  srand(seed);
  for (int step = 0; step < 400 && !ended; step++) {
    const int op = rand() % 8;
    if (op < 4) {  // need, with and without a bound on the read-ahead, then part of it is taken
      const size_t n = op == 3 && bufsize ? s.buf.size() + 1 + rand() % 50 : 1 + rand() % 40;  // (op 3: more than the buffer holds)
      const size_t look = op == 0 ? 0 : op == 1 ? 5 : ~(size_t)0;
      const size_t before = s.avail(), size_before = s.buf.size();
      const bool ok = op == 3 ? s.need(n) : s.need(n, look);
      if (ok) {
        CHECK(s.avail() >= n);
        if (op == 3 && bufsize) CHECK(size_before < n && s.buf.size() >= n);
        CHECK(f.at - P <= std::max(before, n + std::min(look, s.buf.size())));  // never further ahead than n + look
      } else {
        CHECK(s.bad || f.limit - P < n);  // never short while the bytes exist
        CHECK(s.bad == (f.error_call >= 0 && f.calls > f.error_call));
        ended = true;
      }
      held_is_right();
      const size_t take = ok ? rand() % (n + 1) : 0;
      s.skip(take);
      P += take;
    } else if (op < 6) {  // pass: the buffered bytes first, then skip, or reads that are dropped
      const size_t n = rand() % 300, before = s.avail();
      const uint64_t delivered_before = delivered;
      const uint64_t got = s.pass(n);
      CHECK(got <= n && got >= std::min(n, before));
      if (sk == TOO_MUCH && n > before) { CHECK(s.bad && got == before); ended = true; }
      else if (got < n) { CHECK(s.bad || s.eof); CHECK(s.bad || sk == SHORT || P + got == f.limit); ended = true; }
      P += got;
      if (sk != NO_SKIP) CHECK(delivered == delivered_before);  // with a skip callback nothing is read to be dropped
    } else {  // read_into: the buffered bytes first, then the callback straight into the destination
      const size_t n = rand() % 300;
      std::unique_ptr<uint8_t[]> dst(new uint8_t[n ? n : 1]);
      const uint64_t got = s.read_into(dst.get(), n);
      CHECK(got <= n);
      for (size_t i = 0; i < got; i++) CHECK(dst[i] == byte_at(P + i));
      if (got < n) { CHECK(s.bad || P + got == f.limit); ended = true; }
      P += got;
    }
    counters();
  }
  // behind the end nothing more arrives, and nothing is counted twice
  if (ended) {
    const size_t before = s.avail();
    CHECK(!s.need(before + 1) && s.pass(before + 10) == before);
    P += before;
    counters();
  }
  CHECK(wait >= 0);
}

int main() {
  unsigned seed = 1;
  for (Read rd : {ONE_BYTE, ODD_PIECES, ERROR_AT_K, ENDS_EARLY})
    for (Skip sk : {NO_SKIP, EXACT, SHORT, TOO_MUCH})
      for (size_t bufsize : {(size_t)64, (size_t)0})  // 0: the look-ahead buffer as open() makes it
        for (int rep = 0; rep < 6; rep++) drive(rd, sk, bufsize, seed++);
  puts("src_check: ok");
  return 0;
}
