// exceptionstream_check.cpp -- a program of its own over scalce_amd/csrc/exceptionstream.hpp (no device, no library): header
// round trip, every error string, the cursor over read callbacks that deliver 1 byte, 7 bytes and everything at once, ranges
// [r0, r1) that are empty, hold one entry, begin or end on a record without entries, X = 0, and a stream cut at every byte.
// Built by tests/test_exceptions_cpu.py under AddressSanitizer and UBSan; prints "exceptionstream_check: ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scalce_amd/csrc/exceptionstream.hpp"

using namespace scalce_host;

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

static bool is(const char *got, const char *want) { return got && std::string(got) == want; }

struct Source {  // a stream that hands out at most `step` bytes per call (0: everything that is asked for)
  std::vector<uint8_t> data;
  size_t at = 0, step = 0;
  int fail_at_call = -1, calls = 0;
};
static int64_t source_read(void *user, void *dst, uint64_t cap) {
  Source *s = static_cast<Source *>(user);
  if (s->calls++ == s->fail_at_call) return -1;
  size_t k = s->data.size() - s->at;
  if (k > cap) k = (size_t)cap;
  if (s->step && k > s->step) k = s->step;
  if (k) memcpy(dst, s->data.data() + s->at, k);
  s->at += k;
  return (int64_t)k;
}

static std::vector<uint8_t> make_stream(const std::vector<uint64_t> &e, uint32_t L, uint64_t N, int64_t X = -1) {
  std::vector<uint8_t> out(EXCEPTION_HEADER_BYTES + 8 * e.size());
  exception_header_write(out.data(), L, N, X < 0 ? e.size() : (uint64_t)X);
  if (!e.empty()) memcpy(out.data() + EXCEPTION_HEADER_BYTES, e.data(), 8 * e.size());
  return out;
}

// records 0..9 of 50 bases: entries in records 1 (one), 4 (three), 5 (one), 9 (two); none in 0, 2, 3, 6, 7, 8
static std::vector<uint64_t> sample() {
  return {exception_entry(1, 0, 'n', '#'),  exception_entry(4, 0, 'N', '#'),  exception_entry(4, 7, 'a', 'I'), exception_entry(4, 49, 'R', '!'),
          exception_entry(5, 49, 'N', '5'), exception_entry(9, 3, 'c', 0),    exception_entry(9, 4, 'g', 0)};
}
static std::vector<uint64_t> in_range(const std::vector<uint64_t> &e, uint64_t r0, uint64_t r1) {
  std::vector<uint64_t> out;
  for (uint64_t x : e)
    if (exception_record(x) >= r0 && exception_record(x) < r1) out.push_back(x);
  return out;
}

static void entry_fields() {
  const uint64_t e = exception_entry((1ull << 36) - 1, 2498, 'N', '#');
  CHECK((e & 255) == 'N' && ((e >> 8) & 255) == '#' && exception_pos(e) == 2498 && exception_record(e) == (1ull << 36) - 1);
  CHECK(exception_entry(0, 0, 0, 0) == 0 && exception_entry(1, 0, 0, 0) == 1ull << 28 && exception_entry(0, 1, 0, 0) == 1ull << 16);
  CHECK(exception_entry(3, 4095, 255, 255) < exception_entry(4, 0, 0, 0));  // records, then positions, order the entries
}

static void header_round_trip() {
  uint8_t h[EXCEPTION_HEADER_BYTES];
  exception_header_write(h, 100, 12345678901ull, 15607);
  CHECK(!memcmp(h, "scalce22", 8));
  int32_t f[2];
  memcpy(f, h + 8, 8);
  CHECK(f[0] == 8 && f[1] == 100);
  uint32_t L = 7;
  uint64_t n = 7, x = 7;
  CHECK(exception_header_read(h, sizeof h, &L, &n, &x) == nullptr && L == 100 && n == 12345678901ull && x == 15607);
  exception_header_write(h, 1, 0, 0);
  CHECK(exception_header_read(h, sizeof h, &L, &n, &x) == nullptr && L == 1 && n == 0 && x == 0);
  exception_header_write(h, 4095, EXCEPTION_MAX_RECORDS - 1, 1ull << 40);
  CHECK(exception_header_read(h, sizeof h, &L, &n, &x) == nullptr && L == 4095 && n == EXCEPTION_MAX_RECORDS - 1 && x == 1ull << 40);
}

static void header_errors() {
  uint8_t h[EXCEPTION_HEADER_BYTES], g[EXCEPTION_HEADER_BYTES];
  uint32_t L;
  uint64_t n, x;
  exception_header_write(h, 100, 3, 2);
  for (size_t have = 0; have < EXCEPTION_HEADER_BYTES; have++) CHECK(is(exception_header_read(h, have, &L, &n, &x), "truncated exception stream"));
  memcpy(g, h, sizeof h); g[0] = 'x';
  CHECK(is(exception_header_read(g, sizeof g, &L, &n, &x), "is not a scalce exception stream"));
  for (int32_t width : {0, 1, 2, 4, -1}) {  // (the other streams' widths are not this stream's)
    memcpy(g, h, sizeof h); memcpy(g + 8, &width, 4);
    CHECK(is(exception_header_read(g, sizeof g, &L, &n, &x), "is not a scalce exception stream"));
  }
  for (int32_t len : {0, -1, 4096}) {
    memcpy(g, h, sizeof h); memcpy(g + 12, &len, 4);
    CHECK(is(exception_header_read(g, sizeof g, &L, &n, &x), "is not a scalce exception stream"));
  }
  for (int64_t v : {(int64_t)-1, (int64_t)EXCEPTION_MAX_RECORDS}) {
    memcpy(g, h, sizeof h); memcpy(g + 16, &v, 8);
    CHECK(is(exception_header_read(g, sizeof g, &L, &n, &x), "is not a scalce exception stream"));
  }
  const int64_t neg = -1;
  memcpy(g, h, sizeof h); memcpy(g + 24, &neg, 8);
  CHECK(is(exception_header_read(g, sizeof g, &L, &n, &x), "is not a scalce exception stream"));
  char msg[200];
  exception_count_message(msg, sizeof msg, 5, 7);
  CHECK(std::string(msg) == "exception stream holds 5 records, the archive 7");
  exception_length_message(msg, sizeof msg, 100, 150);
  CHECK(std::string(msg) == "exception stream is for reads of 100 bases, the archive's have 150");
}

// every way of cutting the ten records into consecutive ranges of `width` records, over sources of every step
static void cursor_ranges() {
  const std::vector<uint64_t> e = sample();
  for (size_t step : {(size_t)1, (size_t)7, (size_t)0})
    for (size_t bufsz : {(size_t)1, (size_t)5, (size_t)65536})
      for (uint64_t width : {1ull, 2ull, 3ull, 10ull, 64ull}) {
        Source s;
        s.data = make_stream(e, 50, 10);
        s.step = step;
        ExceptionCursor c;
        c.start(source_read, &s, bufsz);
        CHECK(c.read_header() == nullptr && c.read_len == 50 && c.records == 10 && c.total == 7);
        for (uint64_t r0 = 0; r0 < 10; r0 += width) {
          std::vector<uint64_t> got;
          CHECK(c.take(r0, r0 + width, &got) == nullptr);
          CHECK(got == in_range(e, r0, r0 + width));
        }
        CHECK(c.taken == 7);
      }
  // an empty range takes nothing and loses nothing
  {
    Source s;
    s.data = make_stream(e, 50, 10);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr);
    std::vector<uint64_t> got;
    CHECK(c.take(4, 4, &got) == nullptr && got.empty() && c.taken == 1);  // (record 1's entry lies in front of it)
    CHECK(c.take(4, 5, &got) == nullptr && got == in_range(e, 4, 5));
  }
  // a range in the middle: the entries in front of it are passed over, none behind it is taken; it begins (2) and ends (8) on
  // records without entries; then one that holds a single entry
  {
    Source s;
    s.data = make_stream(e, 50, 10);
    s.step = 7;
    ExceptionCursor c;
    c.start(source_read, &s, 16);
    CHECK(c.read_header() == nullptr);
    std::vector<uint64_t> got;
    CHECK(c.take(2, 8, &got) == nullptr && got == in_range(e, 2, 8) && got.size() == 4 && c.taken == 5);
    CHECK(s.at <= EXCEPTION_HEADER_BYTES + 8 * 6 + 16);  // (what lies behind the range is not read: one entry looked at, one buffer)
    got.clear();
    CHECK(c.take(8, 9, &got) == nullptr && got.empty());
    CHECK(c.take(9, 10, nullptr) == nullptr && c.taken == 7);
  }
  {
    Source s;
    s.data = make_stream(e, 50, 10);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr);
    std::vector<uint64_t> got;
    CHECK(c.take(5, 6, &got) == nullptr && got.size() == 1 && got[0] == e[4]);
  }
  // X = 0
  {
    Source s;
    s.data = make_stream({}, 50, 10);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr && c.total == 0);
    std::vector<uint64_t> got;
    CHECK(c.take(0, 10, &got) == nullptr && got.empty());
  }
}

static void cursor_errors() {
  const std::vector<uint64_t> e = sample();
  const std::vector<uint8_t> whole = make_stream(e, 50, 10);
  // cut at every byte: inside the header, inside an entry, between two entries
  for (size_t cut = 0; cut < whole.size(); cut++)
    for (size_t step : {(size_t)1, (size_t)7, (size_t)0}) {
      Source s;
      s.data.assign(whole.begin(), whole.begin() + cut);
      s.step = step;
      ExceptionCursor c;
      c.start(source_read, &s, 9);
      const char *why = c.read_header();
      if (cut < EXCEPTION_HEADER_BYTES) { CHECK(is(why, "truncated exception stream")); continue; }
      CHECK(why == nullptr);
      std::vector<uint64_t> got;
      CHECK(is(c.take(0, 10, &got), "truncated exception stream"));
      CHECK(got.size() == (cut - EXCEPTION_HEADER_BYTES) / 8);
    }
  // entries that do not ascend: a swap, a repeat, the same place of the same record twice with another letter and quality
  for (int kind = 0; kind < 3; kind++) {
    std::vector<uint64_t> bad = e;
    if (kind == 2) bad[3] = exception_entry(4, 7, 'c', 'J');  // (greater as a number than bad[2], the same record and position)
    else if (kind) bad[3] = bad[2]; else std::swap(bad[2], bad[3]);
    if (kind == 2) CHECK(bad[3] > bad[2] && (bad[3] >> 16) == (bad[2] >> 16));
    Source s;
    s.data = make_stream(bad, 50, 10);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr);
    CHECK(is(c.take(0, 10, nullptr), "exception stream: entries are not in ascending order"));
  }
  // an entry outside its record: position = L, record = N
  for (int kind = 0; kind < 2; kind++) {
    std::vector<uint64_t> bad = e;
    bad.back() = kind ? exception_entry(10, 0, 'n', 0) : exception_entry(9, 50, 'n', 0);
    Source s;
    s.data = make_stream(bad, 50, 10);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr);
    std::vector<uint64_t> got;
    CHECK(is(c.take(0, 10, &got), "exception stream: an entry lies outside its record") && got.size() == 6);
  }
  // a read that fails: in the header, behind it
  for (int call : {0, 1}) {
    Source s;
    s.data = whole;
    s.step = 40;
    s.fail_at_call = call;
    ExceptionCursor c;
    c.start(source_read, &s);
    const char *why = c.read_header();
    if (call == 0) { CHECK(is(why, "exception stream: read failed")); continue; }
    CHECK(why == nullptr);
    CHECK(is(c.take(0, 10, nullptr), "exception stream: read failed"));
  }
  // a header that promises more entries than the stream holds, and fewer (what lies behind them is not looked at)
  {
    Source s;
    s.data = make_stream(e, 50, 10, 8);
    ExceptionCursor c;
    c.start(source_read, &s);
    CHECK(c.read_header() == nullptr);
    CHECK(is(c.take(0, 10, nullptr), "truncated exception stream"));
    Source t;
    t.data = make_stream(e, 50, 10, 5);
    ExceptionCursor d;
    d.start(source_read, &t);
    CHECK(d.read_header() == nullptr);
    std::vector<uint64_t> got;
    CHECK(d.take(0, 10, &got) == nullptr && got.size() == 5);
  }
}

int main() {
  entry_fields();
  header_round_trip();
  header_errors();
  cursor_ranges();
  cursor_errors();
  puts("exceptionstream_check: ok");
  return 0;
}
