// commentstream_check.cpp -- a program of its own over scalce_amd/csrc/commentstream.hpp (no device, no library): header round
// trip, every error string, the cursor over read callbacks that deliver 1 byte, 7 bytes and everything at once, entries of 0, 1
// and 65535 bytes, and a three-entry stream cut at every byte.  Built by tests/test_comments_cpu.py under AddressSanitizer and
// UBSan; prints "commentstream_check: ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scalce_amd/csrc/commentstream.hpp"

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
  std::vector<uint8_t> out(COMMENT_HEADER_BYTES);
  comment_header_write(out.data(), longest < 0 ? c : (uint32_t)longest, entries.size());
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

// the stream of `entries` through callbacks of every step and buffers of several sizes: take and skip in several groupings
static void cursor_walks(const std::vector<std::string> &entries) {
  const std::vector<uint8_t> data = make_stream(entries);
  for (size_t step : {(size_t)1, (size_t)7, (size_t)0})
    for (size_t buffer : {(size_t)1, (size_t)5, (size_t)64, (size_t)1 << 16})
      for (size_t group : {(size_t)1, (size_t)2, entries.size() ? entries.size() : 1}) {
        Source s;
        s.data = data; s.step = step;
        CommentCursor cur;
        cur.start(source_read, &s, buffer);
        CHECK(cur.read_header() == nullptr);
        CHECK(cur.total == entries.size());
        std::vector<uint8_t> out;
        size_t k = 0;
        bool skipping = false;
        std::string want;
        while (k < entries.size()) {
          const size_t n = std::min(group, entries.size() - k);
          if (skipping) CHECK(cur.skip(n) == nullptr);
          else { CHECK(cur.take(n, &out) == nullptr); want += body_of(entries, k, n); }
          skipping = !skipping;
          k += n;
          CHECK(cur.taken == k);
        }
        CHECK(std::string(out.begin(), out.end()) == want);
        CHECK(cur.bytes == data.size() - COMMENT_HEADER_BYTES);
        CHECK(cur.take(0, &out) == nullptr);
        CHECK(is(cur.take(1, &out), "truncated comment stream"));  // nothing behind the last entry
        char msg[128];
        CHECK(cur.check_count(entries.size(), msg, sizeof msg) == nullptr);
        CHECK(is(cur.check_count(entries.size() + 1, msg, sizeof msg),
                 ("comment stream holds " + std::to_string(entries.size()) + " entries, the archive " + std::to_string(entries.size() + 1) + " records").c_str()));
      }
}

static void cut_at_every_byte() {
  const std::vector<std::string> entries = {" 1:N:0:ATCACG", "", " "};
  const std::vector<uint8_t> whole = make_stream(entries);
  // where each entry's newline lies
  std::vector<size_t> ends;
  for (size_t i = COMMENT_HEADER_BYTES; i < whole.size(); i++)
    if (whole[i] == '\n') ends.push_back(i);
  CHECK(ends.size() == 3);
  for (size_t cut = 0; cut < whole.size(); cut++)
    for (size_t step : {(size_t)1, (size_t)7, (size_t)0}) {
      Source s;
      s.data.assign(whole.begin(), whole.begin() + cut); s.step = step;
      CommentCursor cur;
      cur.start(source_read, &s, 16);
      const char *e = cur.read_header();
      if (cut < COMMENT_HEADER_BYTES) { CHECK(is(e, "truncated comment stream")); continue; }
      CHECK(e == nullptr && cur.total == 3 && cur.longest == 13);
      size_t complete = 0;  // entries whose newline the cut stream still holds
      for (size_t at : ends) complete += at < cut ? 1 : 0;
      std::vector<uint8_t> out;
      for (size_t k = 0; k < 3; k++) {
        e = cur.take(1, &out);
        if (k < complete) CHECK(e == nullptr);
        else { CHECK(is(e, "truncated comment stream")); break; }
      }
      CHECK(cur.taken == complete);
    }
}

static void entry_longer_than_header() {
  const std::vector<std::string> entries = {" ab", " abcd", " a"};
  for (size_t step : {(size_t)1, (size_t)7, (size_t)0})
    for (size_t buffer : {(size_t)2, (size_t)64}) {
      Source s;
      s.data = make_stream(entries, 4);  // the header says 4, the second entry holds 5
      s.step = step;
      CommentCursor cur;
      cur.start(source_read, &s, buffer);
      CHECK(cur.read_header() == nullptr && cur.longest == 4);
      std::vector<uint8_t> out;
      CHECK(cur.take(1, &out) == nullptr);
      CHECK(is(cur.take(1, &out), "comment stream: an entry is longer than its header says"));
    }
  // an entry exactly as long as the header says passes, in one read and byte by byte
  for (size_t step : {(size_t)1, (size_t)0}) {
    Source s;
    s.data = make_stream(entries, 5);
    s.step = step;
    CommentCursor cur;
    cur.start(source_read, &s, 3);
    CHECK(cur.read_header() == nullptr);
    CHECK(cur.skip(3) == nullptr && cur.taken == 3);
  }
}

static void failed_read() {
  const std::vector<std::string> entries = {" x", " y"};
  // (28 bytes: a failure in the header's first and second read, and one behind the header, inside the entries)
  const size_t steps[3] = {20, 20, 26};
  const int calls[3] = {0, 1, 1};
  for (int i = 0; i < 3; i++) {
    Source s;
    s.data = make_stream(entries);
    s.step = steps[i];
    s.fail_at_call = calls[i];
    CommentCursor cur;
    cur.start(source_read, &s, 64);
    const char *e = cur.read_header();
    if (!e) e = cur.skip(2);
    CHECK(is(e, "comment stream: read failed"));
  }
}

int main() {
  header_round_trip();
  header_errors();
  cursor_walks({});
  cursor_walks({""});
  cursor_walks({" "});
  cursor_walks({"", " ", " 1:N:0:ATCACG", "", " length=100"});
  cursor_walks({std::string(65535, 'q'), "", "x", std::string(65535, ' ')});
  cut_at_every_byte();
  entry_longer_than_header();
  failed_read();
  puts("commentstream_check: ok");
  return 0;
}
