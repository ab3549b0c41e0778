// plusstream_check.cpp -- a program of its own over scalce_amd/csrc/plusstream.hpp (no device, no library): header round trip,
// the P = 0 form, every error string, the class of an entry and what it adds to a record, the cursor over read callbacks that
// deliver 1 byte, 7 bytes and everything at once, entries of 0, 1 and 65535 bytes, a stream cut at every byte and every kind
// of malformed entry.  Built by tests/test_plus_cpu.py under AddressSanitizer and UBSan; prints "plusstream_check: ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scalce_amd/csrc/plusstream.hpp"

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

static std::vector<uint8_t> make_stream(const std::vector<std::string> &entries, int64_t longest = -1) {
  uint32_t c = 0;
  for (const std::string &e : entries) c = e.size() > c ? (uint32_t)e.size() : c;
  std::vector<uint8_t> out(PLUS_HEADER_BYTES);
  plus_header_write(out.data(), longest < 0 ? c : (uint32_t)longest, entries.size());
  if (!c && longest <= 0) return out;  // the P = 0 form: the header alone
  for (const std::string &e : entries) {
    out.insert(out.end(), e.begin(), e.end());
    out.push_back('\n');
  }
  return out;
}
static std::string body_of(const std::vector<std::string> &entries, size_t first, size_t n) {
  std::string s;
  for (size_t i = first; i < first + n; i++) s += entries[i] + "\n";
  return s;
}

static void header_round_trip() {
  uint8_t h[PLUS_HEADER_BYTES];
  plus_header_write(h, 40, 4000000000ull);
  CHECK(!memcmp(h, "scalce22", 8));
  int32_t f[2];
  memcpy(f, h + 8, 8);
  CHECK(f[0] == 0 && f[1] == 40);
  uint32_t p = 7;
  uint64_t n = 7;
  CHECK(plus_header_read(h, sizeof h, &p, &n) == nullptr && p == 40 && n == 4000000000ull);
  plus_header_write(h, 0, 0);
  CHECK(plus_header_read(h, sizeof h, &p, &n) == nullptr && p == 0 && n == 0);
  plus_header_write(h, 65535, 0xFFFFFFFFull);
  CHECK(plus_header_read(h, sizeof h, &p, &n) == nullptr && p == 65535 && n == 0xFFFFFFFFull);
}

static void header_errors() {
  uint8_t h[PLUS_HEADER_BYTES], g[PLUS_HEADER_BYTES];
  uint32_t p;
  uint64_t n;
  plus_header_write(h, 12, 3);
  for (size_t have = 0; have < PLUS_HEADER_BYTES; have++) CHECK(is(plus_header_read(h, have, &p, &n), "truncated plus-line stream"));
  memcpy(g, h, sizeof h); g[0] = 'x';
  CHECK(is(plus_header_read(g, sizeof g, &p, &n), "is not a scalce plus-line stream"));
  for (int32_t width : {1, 2, 4, 8, -1}) {  // (the other streams' widths are not this stream's)
    memcpy(g, h, sizeof h); memcpy(g + 8, &width, 4);
    CHECK(is(plus_header_read(g, sizeof g, &p, &n), "is not a scalce plus-line stream"));
  }
  for (int32_t longest : {-1, 65536}) {
    memcpy(g, h, sizeof h); memcpy(g + 12, &longest, 4);
    CHECK(is(plus_header_read(g, sizeof g, &p, &n), "is not a scalce plus-line stream"));
  }
  for (int64_t count : {(int64_t)-1, (int64_t)1 << 32}) {
    memcpy(g, h, sizeof h); memcpy(g + 16, &count, 8);
    CHECK(is(plus_header_read(g, sizeof g, &p, &n), "is not a scalce plus-line stream"));
  }
  char msg[200];
  plus_count_message(msg, sizeof msg, 5, 7);
  CHECK(is(msg, "plus-line stream holds 5 entries, the archive 7 records"));
  CHECK(is(plus_entry_too_long(), "plus-line stream: an entry is longer than its header says"));
  CHECK(is(plus_malformed(), "plus-line stream: malformed entry"));
}

static void classes() {
  auto cls = [](const std::string &e) { return plus_class(reinterpret_cast<const uint8_t *>(e.data()), e.size()); };
  CHECK(cls("") == PLUS_BARE);
  CHECK(cls("=") == PLUS_REPEAT);
  CHECK(cls("'a") == PLUS_LITERAL && cls("'=") == PLUS_LITERAL && cls("''") == PLUS_LITERAL && cls("'= x") == PLUS_LITERAL);
  CHECK(cls("'") == PLUS_MALFORMED);  // an empty literal is the bare line: it cannot be
  CHECK(cls("=a") == PLUS_MALFORMED && cls("==") == PLUS_MALFORMED && cls("a") == PLUS_MALFORMED && cls("+a") == PLUS_MALFORMED &&
        cls(" ") == PLUS_MALFORMED);
  CHECK(plus_growth(PLUS_BARE, 0, 30) == 0 && plus_growth(PLUS_REPEAT, 1, 30) == 30 && plus_growth(PLUS_LITERAL, 5, 30) == 4 &&
        plus_growth(PLUS_MALFORMED, 5, 30) == 0);
}

static void walks() {
  std::vector<std::string> entries = {"=", "", "'SRR001666.1 length=36", "'=", "", "=", std::string("'") + std::string(65534, 'q'), "''x"};
  const std::vector<uint8_t> data = make_stream(entries);
  for (size_t step : {(size_t)1, (size_t)7, (size_t)0})
    for (size_t buffer : {(size_t)1, (size_t)5, (size_t)1 << 16}) {
      Source s;
      s.data = data; s.step = step;
      PlusCursor c;
      c.start(source_read, &s, buffer);
      CHECK(c.read_header() == nullptr && c.longest == 65535 && c.total == entries.size());
      std::vector<uint8_t> out;
      CHECK(c.skip(2) == nullptr && c.taken == 2);         // a range passes over what lies in front of it
      CHECK(c.take(3, &out) == nullptr && c.taken == 5);
      CHECK(std::string(out.begin(), out.end()) == body_of(entries, 2, 3));
      out.clear();
      CHECK(c.take(0, &out) == nullptr && out.empty());
      CHECK(c.take(3, &out) == nullptr && c.taken == 8);
      CHECK(std::string(out.begin(), out.end()) == body_of(entries, 5, 3));
      CHECK(c.repeats == 2 && c.literals == 4);
      CHECK(is(c.take(1, &out), "truncated plus-line stream"));
      char msg[200];
      CHECK(c.check_count(entries.size(), msg, sizeof msg) == nullptr);
      CHECK(is(c.check_count(9, msg, sizeof msg), "plus-line stream holds 8 entries, the archive 9 records"));
    }
}

static void no_entries_form() {
  const std::vector<uint8_t> data = make_stream({"", "", "", ""});
  CHECK(data.size() == PLUS_HEADER_BYTES);
  Source s;
  s.data = data;
  PlusCursor c;
  c.start(source_read, &s);
  CHECK(c.read_header() == nullptr && c.longest == 0 && c.total == 4);
  std::vector<uint8_t> out;
  CHECK(c.skip(1) == nullptr && c.take(3, &out) == nullptr && c.taken == 4);
  CHECK(std::string(out.begin(), out.end()) == "\n\n\n");
  CHECK(s.calls == 1);  // nothing is read behind the header
  char msg[200];
  CHECK(c.check_count(4, msg, sizeof msg) == nullptr && is(c.check_count(5, msg, sizeof msg), "plus-line stream holds 4 entries, the archive 5 records"));
}

static void cut_at_every_byte() {
  const std::vector<std::string> entries = {"'ab", "", "="};
  const std::vector<uint8_t> whole = make_stream(entries);
  for (size_t cut = 0; cut < whole.size(); cut++)
    for (size_t step : {(size_t)1, (size_t)0}) {
      Source s;
      s.data.assign(whole.begin(), whole.begin() + cut);
      s.step = step;
      PlusCursor c;
      c.start(source_read, &s, 4);
      const char *why = c.read_header();
      if (cut < PLUS_HEADER_BYTES) { CHECK(is(why, "truncated plus-line stream")); continue; }
      CHECK(why == nullptr);
      std::vector<uint8_t> out;
      CHECK(is(c.take(3, &out), "truncated plus-line stream"));
      // what came before the cut was handed out whole
      const std::string body = body_of(entries, 0, 3);
      CHECK(out.size() <= cut - PLUS_HEADER_BYTES && std::string(out.begin(), out.end()) == body.substr(0, out.size()));
    }
}

static void bad_entries() {
  for (const char *e : {"x", "=x", "'", "+r1", " "}) {
    Source s;
    s.data = make_stream({"=", e, ""}, 8);
    for (size_t step : {(size_t)1, (size_t)0}) {
      s.at = 0; s.calls = 0; s.step = step;
      PlusCursor c;
      c.start(source_read, &s, 3);
      CHECK(c.read_header() == nullptr);
      CHECK(c.take(1, nullptr) == nullptr);
      CHECK(is(c.take(2, nullptr), "plus-line stream: malformed entry"));
    }
  }
  {  // an entry that outgrows the header's P, whether its newline is in the buffer or not
    for (size_t buffer : {(size_t)2, (size_t)64}) {
      Source s;
      s.data = make_stream({"'abc", "="}, 3);
      PlusCursor c;
      c.start(source_read, &s, buffer);
      CHECK(c.read_header() == nullptr);
      CHECK(is(c.take(2, nullptr), "plus-line stream: an entry is longer than its header says"));
    }
  }
  {  // a read that fails, in the header and behind it
    Source s;
    s.data = make_stream({"=", "'a"});
    s.fail_at_call = 0;
    PlusCursor c;
    c.start(source_read, &s);
    CHECK(is(c.read_header(), "plus-line stream: read failed"));
    Source t;
    t.data = s.data; t.step = PLUS_HEADER_BYTES; t.fail_at_call = 1;
    c.start(source_read, &t);
    CHECK(c.read_header() == nullptr);
    CHECK(is(c.take(1, nullptr), "plus-line stream: read failed"));
  }
}

int main() {
  header_round_trip();
  header_errors();
  classes();
  walks();
  no_entries_form();
  cut_at_every_byte();
  bad_entries();
  puts("plusstream_check: ok");
  return 0;
}
