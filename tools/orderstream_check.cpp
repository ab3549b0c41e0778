// orderstream_check.cpp -- the host side of the order stream (scalce_amd/csrc/orderstream.hpp: header, error strings, entry
// checks, the stripe plan, the table of the spill's shares, its record word and its file) on its own: a program for AddressSanitizer, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/orderstream_check.cpp -o /tmp/oc && /tmp/oc
// Every array handed to the code under test is a heap block of exactly the size it may touch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../scalce_amd/csrc/orderstream.hpp"

using namespace scalce_host;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void header_round_trip() {
  for (uint64_t n : {0ull, 1ull, 3000ull, 0xFFFFFFFFull}) {
    std::unique_ptr<uint8_t[]> h(new uint8_t[ORDER_HEADER_BYTES]);
    order_header_write(h.get(), n);
    CHECK(!memcmp(h.get(), "scalce22", 8));
    int32_t f[2];
    memcpy(f, h.get() + 8, 8);
    CHECK(f[0] == 4 && f[1] == 0);
    uint64_t back = ~0ull;
    CHECK(order_header_read(h.get(), ORDER_HEADER_BYTES, &back) == nullptr && back == n);
  }
}
static void header_errors() {
  std::unique_ptr<uint8_t[]> h(new uint8_t[ORDER_HEADER_BYTES]);
  uint64_t n = 7;
  order_header_write(h.get(), 5);
  for (size_t have = 0; have < ORDER_HEADER_BYTES; have++) {  // cut anywhere inside the header (the bytes behind are not read)
    std::unique_ptr<uint8_t[]> cut(new uint8_t[have ? have : 1]);
    memcpy(cut.get(), h.get(), have);
    const char *why = order_header_read(cut.get(), have, &n);
    CHECK(why && !strcmp(why, "truncated order stream") && n == 7);
  }
  auto refused = [&](size_t at, uint8_t v) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[ORDER_HEADER_BYTES]);
    memcpy(b.get(), h.get(), ORDER_HEADER_BYTES);
    b[at] = v;
    const char *why = order_header_read(b.get(), ORDER_HEADER_BYTES, &n);
    return why && !strcmp(why, "is not a scalce order stream");
  };
  CHECK(refused(0, 'x'));    // the magic
  CHECK(refused(8, 2));      // a width that is not 4
  CHECK(refused(8, 8));
  CHECK(refused(12, 1));     // the reserved word
  CHECK(refused(23, 0x80));  // a negative count
  CHECK(refused(20, 1));     // more records than a u32 entry can name
  CHECK(!refused(7, '3'));   // (the last magic byte is the minor version, as for the other streams)
  CHECK(!strcmp(order_not_permutation(), "order stream is not a permutation of the records"));
  char msg[128];
  order_count_message(msg, sizeof msg, 2999, 3000);
  CHECK(!strcmp(msg, "order stream holds 2999 entries, the archive 3000 records"));
}
static void entry_checks() {
  std::unique_ptr<uint32_t[]> e(new uint32_t[5]{4, 0, 3, 1, 2});
  CHECK(order_entries_in_range(e.get(), 5, 5));
  CHECK(!order_entries_in_range(e.get(), 5, 4));
  CHECK(order_entries_in_range(e.get(), 0, 0));
  e[2] = 5;
  CHECK(!order_entries_in_range(e.get(), 5, 5));
}
static void plan() {
  uint64_t o[2];
  order_plan(3000, 1, 500, o);              CHECK(o[0] == 1 && o[1] == 3000);      // a window below one record
  order_plan(3000, 3000 * 500, 500, o);     CHECK(o[0] == 3000 && o[1] == 1);      // the window is the archive
  order_plan(3000, 1ull << 30, 500, o);     CHECK(o[0] == (1ull << 30) / 500 && o[1] == 1);
  order_plan(0, 1000, 500, o);              CHECK(o[0] == 2 && o[1] == 0);
  order_plan(1, 1, 500, o);                 CHECK(o[0] == 1 && o[1] == 1);
  order_plan(65536, 1, 500, o);             CHECK(o[0] == 1 && o[1] == 65536);     // the cap, just reached
  order_plan(65537, 1, 500, o);             CHECK(o[0] == 2 && o[1] == 32769);     // ... and raised R
  order_plan(0xFFFFFFFFull, 1, 500, o);     CHECK(o[1] <= ORDER_MAX_STRIPES && o[0] * o[1] >= 0xFFFFFFFFull);
  for (int t = 0; t < 2000; t++) {
    const uint64_t N = rnd() % 300000, W = 1 + rnd() % 100000, rec = 1 + rnd() % 700;
    order_plan(N, W, rec, o);
    CHECK(o[0] >= 1 && o[1] == (N + o[0] - 1) / o[0] && o[1] <= ORDER_MAX_STRIPES);
    const uint64_t plain = W / rec < 1 ? 1 : W / rec;
    if (o[0] != plain) CHECK(o[0] > plain && (N + plain - 1) / plain > ORDER_MAX_STRIPES);  // only the cap raises R
    else if (W >= rec) CHECK(o[0] * rec <= W);
  }
}

// W windows over S stripes: every window's records get random stripes, are grouped, and the pieces the table hands out per
// stripe must be exactly the byte and record ranges of a reference made record by record
static void table_case(uint64_t W, uint64_t S, uint64_t per_window, bool sparse) {
  struct Rec { uint64_t stripe, bytes, text_at, rec_at; };
  StripeTable t;
  t.reset(S);
  std::vector<std::vector<std::vector<Rec>>> want(S, std::vector<std::vector<Rec>>(W));  // [stripe][window]
  uint64_t text_at = 0, rec_at = 0;
  for (uint64_t w = 0; w < W; w++) {
    const uint64_t n = sparse && w % 2 ? 0 : per_window;  // (windows without records: shares that are all empty)
    std::vector<Rec> recs(n);
    for (auto &r : recs) { r.stripe = sparse ? (rnd() % 3 ? S - 1 : rnd() % S) : rnd() % S; r.bytes = rnd() % 300; }
    std::unique_ptr<uint32_t[]> counts(new uint32_t[S ? S : 1]());
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    uint64_t k = 0;
    off[0] = 0;
    for (uint64_t s = 0; s < S; s++)
      for (auto &r : recs)
        if (r.stripe == s) {
          counts[s]++;
          r.text_at = text_at + off[k]; r.rec_at = rec_at + k;
          off[k + 1] = off[k] + r.bytes;
          want[s][w].push_back(r);
          k++;
        }
    CHECK(k == n && t.add_window(counts.get(), off.get(), n));
    text_at += off[n]; rec_at += n;
  }
  CHECK(t.text_bytes == text_at && t.records == rec_at);
  std::vector<StripeTable::Piece> pieces;
  uint64_t seen = 0;
  for (uint64_t s = 0; s < S; s++) {
    uint64_t bytes = 0, by = 0, rc = 0;
    const uint64_t m = t.take_stripe(pieces, &bytes);
    size_t p = 0;
    for (uint64_t w = 0; w < W; w++) {
      const auto &v = want[s][w];
      if (v.empty()) continue;  // an empty share gives no piece
      CHECK(p < pieces.size());
      uint64_t b = 0;
      for (const auto &r : v) b += r.bytes;
      CHECK(pieces[p].text_at == v[0].text_at && pieces[p].record_at == v[0].rec_at && pieces[p].records == v.size() && pieces[p].bytes == b);
      by += b; rc += v.size(); p++;
    }
    CHECK(p == pieces.size() && m == rc && bytes == by);
    seen += m;
  }
  CHECK(seen == rec_at);
}
static void table_refuses() {
  StripeTable t;
  t.reset(3);
  std::unique_ptr<uint32_t[]> counts(new uint32_t[3]{1, 0, 1});
  std::unique_ptr<uint64_t[]> off(new uint64_t[4]{0, 10, 20, 30});
  CHECK(!t.add_window(counts.get(), off.get(), 3));  // counts that say fewer records than the window holds
  counts[1] = 2;
  CHECK(!t.add_window(counts.get(), off.get(), 3));  // ... or more: nothing behind off[n] is read
  counts[1] = 1;
  CHECK(t.add_window(counts.get(), off.get(), 3) && t.records == 3 && t.text_bytes == 30);
}

// the record word, and the spill file: write and read across a piece boundary, emptied between passes, a read past the end
static void spill_file() {
  CHECK(record_word(0xFFFFFFFFu, 5) == 0x5FFFFFFFFull && record_entry(0x5FFFFFFFFull) == 0xFFFFFFFFu && record_size(0x5FFFFFFFFull) == 5);
  CHECK(record_word(7, 0xFFFFFFFFull) == 0xFFFFFFFF00000007ull && record_size(0xFFFFFFFF00000007ull) == 0xFFFFFFFFull);
  const char *tmp = getenv("TMPDIR");
  const std::string dir = tmp && tmp[0] ? tmp : "/tmp";
  const char *what = nullptr;
  SpillFile none;
  CHECK(!none.reset(dir + "/no_such_directory_of_the_check", &what) && !strcmp(what, "make") && errno == ENOENT && none.fd < 0);
  SpillFile f;
  CHECK(f.reset(dir, &what) && f.fd >= 0);
  f.piece = 7;  // pieces of 7 bytes: 20 bytes go in three calls
  std::unique_ptr<uint8_t[]> out(new uint8_t[20]), back(new uint8_t[20]), part(new uint8_t[9]);
  for (int i = 0; i < 20; i++) out[i] = (uint8_t)(100 + i);
  CHECK(f.transfer(true, out.get(), 20, 3) && lseek(f.fd, 0, SEEK_END) == 23);
  CHECK(f.transfer(false, back.get(), 20, 3) && !memcmp(back.get(), out.get(), 20));
  CHECK(f.transfer(false, part.get(), 9, 3 + 6) && !memcmp(part.get(), out.get() + 6, 9));  // (across the boundary between two pieces)
  CHECK(f.transfer(false, part.get(), 0, 1000));                                            // nothing asked, nothing read
  errno = 0;
  CHECK(!f.transfer(false, back.get(), 20, 4) && errno == EIO);  // one byte past the end
  const int fd = f.fd;
  CHECK(f.reset(dir, &what) && f.fd == fd && lseek(f.fd, 0, SEEK_END) == 0);  // the next pass: the same file, empty
  errno = 0;
  CHECK(!f.transfer(false, back.get(), 1, 0) && errno == EIO);
  CHECK(f.transfer(true, out.get(), 5, 0) && f.transfer(false, back.get(), 5, 0) && !memcmp(back.get(), out.get(), 5));
}

int main() {
  header_round_trip();
  header_errors();
  entry_checks();
  plan();
  for (uint64_t W = 1; W <= 4; W++)
    for (uint64_t S = 1; S <= 5; S++)
      for (int sparse = 0; sparse < 2; sparse++) table_case(W, S, 1 + (W * 7 + S * 3) % 11, sparse);
  table_case(3, 65536, 500, false);
  table_case(2, 65536, 40, true);
  table_case(1, 1, 0, false);
  table_refuses();
  spill_file();
  puts("orderstream_check: ok");
  return 0;
}
