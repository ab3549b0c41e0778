// plusstream_check.cpp -- a program of its own over scalce_amd/csrc/plusstream.hpp (no device, no library): header round trip,
// every error string, the class of an entry and what it adds to a record.  (The entries are walked in archive_walk.hpp:
// tools/archive_walk_check.cpp drives that walk.)  Built by tests/test_plus_cpu.py under AddressSanitizer and UBSan; prints
// "plusstream_check: ok".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../scalce_amd/csrc/plusstream.hpp"

using namespace scalce_host;

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

static bool is(const char *got, const char *want) { return got && std::string(got) == want; }

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

int main() {
  header_round_trip();
  header_errors();
  classes();
  puts("plusstream_check: ok");
  return 0;
}
