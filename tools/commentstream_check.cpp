// commentstream_check.cpp -- a program of its own over scalce_amd/csrc/commentstream.hpp (no device, no library): header round
// trip and every error string.  (The entries are walked in archive_walk.hpp: tools/archive_walk_check.cpp drives that walk.)
// Built by tests/test_comments_cpu.py under AddressSanitizer and UBSan; prints "commentstream_check: ok".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../scalce_amd/csrc/commentstream.hpp"

using namespace scalce_host;

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

static bool is(const char *got, const char *want) { return got && std::string(got) == want; }

static void header_round_trip() {
  uint8_t h[COMMENT_HEADER_BYTES];
  comment_header_write(h, 40, 123456789012ull & 0xFFFFFFFFull);
  CHECK(!memcmp(h, "scalce22", 8));
  int32_t f[2];
  memcpy(f, h + 8, 8);
  CHECK(f[0] == 0 && f[1] == 40);
  uint32_t c = 7;
  uint64_t n = 7;
  CHECK(comment_header_read(h, sizeof h, &c, &n) == nullptr && c == 40 && n == (123456789012ull & 0xFFFFFFFFull));
  comment_header_write(h, 0, 0);
  CHECK(comment_header_read(h, sizeof h, &c, &n) == nullptr && c == 0 && n == 0);
  comment_header_write(h, 65535, 0xFFFFFFFFull);
  CHECK(comment_header_read(h, sizeof h, &c, &n) == nullptr && c == 65535 && n == 0xFFFFFFFFull);
}

static void header_errors() {
  uint8_t h[COMMENT_HEADER_BYTES], g[COMMENT_HEADER_BYTES];
  uint32_t c;
  uint64_t n;
  comment_header_write(h, 12, 3);
  for (size_t have = 0; have < COMMENT_HEADER_BYTES; have++) CHECK(is(comment_header_read(h, have, &c, &n), "truncated comment stream"));
  memcpy(g, h, sizeof h); g[0] = 'x';
  CHECK(is(comment_header_read(g, sizeof g, &c, &n), "is not a scalce comment stream"));
  for (int32_t width : {1, 2, 4, -1}) {  // (the length and order streams' widths are not this stream's)
    memcpy(g, h, sizeof h); memcpy(g + 8, &width, 4);
    CHECK(is(comment_header_read(g, sizeof g, &c, &n), "is not a scalce comment stream"));
  }
  for (int32_t longest : {-1, 65536}) {
    memcpy(g, h, sizeof h); memcpy(g + 12, &longest, 4);
    CHECK(is(comment_header_read(g, sizeof g, &c, &n), "is not a scalce comment stream"));
  }
  for (int64_t count : {(int64_t)-1, (int64_t)1 << 32}) {
    memcpy(g, h, sizeof h); memcpy(g + 16, &count, 8);
    CHECK(is(comment_header_read(g, sizeof g, &c, &n), "is not a scalce comment stream"));
  }
  char msg[128];
  comment_count_message(msg, sizeof msg, 5, 7);
  CHECK(std::string(msg) == "comment stream holds 5 entries, the archive 7 records");
  CHECK(is(comment_truncated(), "truncated comment stream"));
  CHECK(is(comment_not_a_stream(), "is not a scalce comment stream"));
  CHECK(is(comment_entry_too_long(), "comment stream: an entry is longer than its header says"));
}

int main() {
  header_round_trip();
  header_errors();
  puts("commentstream_check: ok");
  return 0;
}
