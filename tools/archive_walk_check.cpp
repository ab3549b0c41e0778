// archive_walk_check.cpp -- the walk over an archive's streams (scalce_amd/csrc/archive_walk.hpp: headers, mate 1's buckets,
// one function per stream that moves it on by n records into a destination or to nowhere, names, the entries of the comment
// and plus-line streams that go with them, the hop over coded frames) on its own: a program for AddressSanitizer, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/archive_walk_check.cpp -o /tmp/awc && /tmp/awc
// The streams are built in memory and come through callbacks that hand out one byte, or odd-sized pieces; what the walk must
// make of them is written out here by hand (bytes, directory entries, and the literal text of every failure), and every
// destination is a heap block of exactly the size the call may touch, so a byte too far is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../scalce_amd/csrc/archive_walk.hpp"

using namespace scalce_host;
typedef std::vector<u8> Bytes;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// ---- the streams behind their callbacks ----------------------------------------------------------------------------------------
enum Read { ONE_BYTE, ODD_PIECES, SEVEN_BYTES, EVERYTHING };
enum Skip { NO_SKIP, EXACT, SHORT };
struct Feed {
  Bytes bytes;
  Read rd = ODD_PIECES;
  Skip sk = NO_SKIP;
  int error_call = -1, calls = 0;
  size_t at = 0;
  static int64_t read_cb(void *user, void *dst, uint64_t cap) {
    Feed &f = *static_cast<Feed *>(user);
    static const size_t odd[5] = {3, 7, 1, 13, 5};
    CHECK(cap > 0);
    if (f.calls++ == f.error_call) return -1;
    size_t k = f.rd == ONE_BYTE ? 1 : f.rd == SEVEN_BYTES ? 7 : f.rd == EVERYTHING ? (size_t)cap : odd[f.calls % 5];
    k = std::min<size_t>(std::min<size_t>(k, cap), f.bytes.size() - f.at);
    std::unique_ptr<u8[]> piece(new u8[k ? k : 1]);  // (what the callback writes is all it may write)
    if (k) memcpy(piece.get(), f.bytes.data() + f.at, k);  // (a stream cut to nothing has no bytes to point at)
    memcpy(dst, piece.get(), k);
    f.at += k;
    return (int64_t)k;
  }
  static int64_t skip_cb(void *user, uint64_t n) {
    Feed &f = *static_cast<Feed *>(user);
    size_t k = std::min<size_t>(n, f.bytes.size() - f.at);
    if (f.sk == SHORT) k /= 2;  // fewer than asked: the stream ends there
    f.at += k;
    return (int64_t)k;
  }
};

template <typename T> void put(Bytes &b, T v) { u8 t[sizeof(T)]; memcpy(t, &v, sizeof(T)); b.insert(b.end(), t, t + sizeof(T)); }
static void put(Bytes &b, const char *s) { b.insert(b.end(), s, s + strlen(s)); }
static void put(Bytes &b, const Bytes &o) { b.insert(b.end(), o.begin(), o.end()); }
static Bytes cut(Bytes b, size_t n) { CHECK(n <= b.size()); b.resize(n); return b; }

// a core table of two cores, of length 3 and 4
static const char *const CORES[2] = {"ACG", "ACGT"};
static int core_length(void *, int core) { CHECK(core >= 0 && core < 2); return (int)strlen(CORES[core]); }
static const char *core_string(void *, int core) { CHECK(core >= 0 && core < 2); return CORES[core]; }

static Bytes reads_header(int32_t L, int32_t no_ac = 0) { Bytes b; put(b, "scalce22"); put(b, no_ac); put(b, L); return b; }
static Bytes bucket_header(int32_t core, uint64_t count) { Bytes b; put(b, core); put(b, count); return b; }
static Bytes names_of_library() { Bytes b; put(b, "scalce22"); put(b, (u8)0); put(b, (int64_t)0); put(b, "lib"); return b; }
static Bytes names_header() { Bytes b; put(b, "scalce22"); put(b, (u8)1); return b; }
static Bytes quality_header() { Bytes b; put(b, "scalce22"); put(b, (int64_t)33); return b; }
static Bytes length_header(int32_t width, int32_t L) { Bytes b; put(b, "scalce22"); put(b, width); put(b, L); return b; }

// an archive: its streams, and the walk opened on them
struct Arc {
  Feed r[2], n[2], q[2], l[2], c[2], p[2];
  bool has_l = false, has_c = false, has_p = false;  // the length, comment and plus-line streams
  int mates = 1, interleave = 0;
  ArcMate am[2];
  Walk w;
  Failure f;
  double wait = 0;
  scalce_unpack_range_stats RS;
  explicit Arc(int L = 5, int no_ac = 0) {
    for (int m = 0; m < 2; m++) { r[m].bytes = reads_header(L, no_ac); n[m].bytes = names_of_library(); q[m].bytes = quality_header(); }
  }
  void feed(Read rd, Skip sk) {
    for (Feed *s : {r, n, q, l, c, p})
      for (int m = 0; m < 2; m++) { s[m].rd = rd; s[m].sk = sk; }
  }
  int open() {
    scalce_unpack_params P;
    scalce_unpack_range RG;
    memset(&P, 0, sizeof P);
    memset(&RG, 0, sizeof RG);
    memset(&RS, 0, sizeof RS);
    P.mates = mates; P.interleave = interleave;
    RG.nrecords = ~0ull;
    scalce_read_fn rd[2][3];
    void *user[2][3];
    for (int m = 0; m < 2; m++) {
      Feed *s[3] = {&r[m], &n[m], &q[m]};
      for (int k = 0; k < 3; k++) { rd[m][k] = Feed::read_cb; user[m][k] = s[k]; RG.skip[m][k] = s[k]->sk == NO_SKIP ? nullptr : Feed::skip_cb; }
      if (has_l) { P.len_rd[m] = Feed::read_cb; P.len_user[m] = &l[m]; P.len_skip[m] = l[m].sk == NO_SKIP ? nullptr : Feed::skip_cb; }
      w.M[m] = &am[m];
    }
    w.cores.count = 2; w.cores.length = core_length; w.cores.string = core_string;
    w.m0 = 0; w.m1 = interleave ? 1 : 0;
    int rc = w.headers(P, RG, rd, user, &wait, RS, f);
    for (int m = 0; m < mates && !rc && has_c; m++) rc = w.text_open(m, am[m].com, Feed::read_cb, &c[m], &wait, f);
    for (int m = 0; m < mates && !rc && has_p; m++) rc = w.text_open(m, am[m].plus, Feed::read_cb, &p[m], &wait, f);
    return rc;
  }
  // the text-entry stream of a kind, and its feed
  TextStream &text(bool plus, int m = 0) { return plus ? am[m].plus : am[m].com; }
  Feed &text_feed(bool plus, int m = 0) { return plus ? p[m] : c[m]; }
};

static void failed_with(int rc, const Failure &f, int mate, int stream, int wants_file, const char *msg, int line) {
  if (rc == SCALCE_ERR_FORMAT && f.rc == rc && f.mate == mate && f.stream == stream && f.wants_file == wants_file && f.msg == msg) return;
  fprintf(stderr, "FAILED %s:%d: rc %d, failure {%d, mate %d, stream %d, wants_file %d, \"%s\"}\n", __FILE__, line, rc, f.rc, f.mate, f.stream,
          f.wants_file, f.msg.c_str());
  exit(1);
}
#define FAILED_WITH(rc, f, mate, stream, wants_file, msg) failed_with((rc), (f), (mate), (stream), (wants_file), (msg), __LINE__)

// ---- the read stream: seven records in four buckets ------------------------------------------------------------------------------
// the root bucket (records 0, 1), a bucket of core 1 without records, core 0 (records 2, 3, 4), core 1 (records 5, 6)
static const struct { int32_t core; uint64_t count; } BUCKETS[4] = {{SCALCE_ROOT_CORE, 2}, {1, 0}, {0, 3}, {1, 2}};
struct Shape {           // what the read length makes of them, worked out by hand:
  int L;
  u32 rb[3];             // bytes per record in the root bucket, under core 0 and under core 1: (L - core + 3) / 4 + (L > 255 ? 2 : 1)
  u64 off_w2, off_w7[2]; // where bucket 3 begins in the window of records 4, 5; where buckets 2 and 3 begin in the window of all
};
static const Shape SHAPES[2] = {{5, {3, 2, 2}, 2 + 12, {6 + 12, 6 + 12 + 6 + 12}},
                                {256, {66, 66, 65}, 66 + 12, {132 + 12, 132 + 12 + 198 + 12}}};
static const int REC_BUCKET[7] = {0, 0, 2, 2, 2, 3, 3};
static u32 rec_bytes(const Shape &s, int i) { return s.rb[REC_BUCKET[i] == 0 ? 0 : REC_BUCKET[i] == 2 ? 1 : 2]; }
static u32 rec_core_len(int i) { return REC_BUCKET[i] == 0 ? 0 : REC_BUCKET[i] == 2 ? 3 : 4; }
static u8 rec_byte(int i, u32 j) { return (u8)(0xA0 + 16 * i + j); }
static Bytes record(const Shape &s, int i) { Bytes b; for (u32 j = 0; j < rec_bytes(s, i); j++) b.push_back(rec_byte(i, j)); return b; }
static Bytes read_stream(const Shape &s) {
  Bytes b = reads_header(s.L);
  int i = 0;
  for (const auto &bk : BUCKETS) {
    put(b, bucket_header(bk.core, bk.count));
    for (uint64_t k = 0; k < bk.count; k++) put(b, record(s, i++));
  }
  return b;
}
// the stream for L = 5, and what the window of all seven records holds of it, byte by byte
static const u8 L5_STREAM[] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2', 0, 0, 0, 0, 5, 0, 0, 0,
                               0xFF, 0xFF, 0xFF, 0x3F, 2, 0, 0, 0, 0, 0, 0, 0, 0xA0, 0xA1, 0xA2, 0xB0, 0xB1, 0xB2,
                               1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                               0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0xC0, 0xC1, 0xD0, 0xD1, 0xE0, 0xE1,
                               1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0xF0, 0xF1, 0x00, 0x01};
static const u8 L5_SLICE_OF_ALL[] = {0xA0, 0xA1, 0xA2, 0xB0, 0xB1, 0xB2, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0xC0, 0xC1, 0xD0, 0xD1, 0xE0, 0xE1,
                                     1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0xF0, 0xF1, 0x00, 0x01};

struct XDir { u64 first, off; u32 core_len, rec_bytes; const char *core; };
struct XWin { u64 got; std::vector<XDir> dir; std::vector<int> segs; };  // segs: a record, or -1 - b: the 12-byte header of bucket b
static std::vector<XWin> expected_windows(const Shape &s, u64 n) {
  const XDir root{0, 0, 0, s.rb[0], ""}, c0{0, 0, 3, s.rb[1], "ACG"}, c1{0, 0, 4, s.rb[2], "ACGT"};
  if (n == 1) return {{1, {root}, {0}}, {1, {root}, {1}}, {1, {c0}, {2}}, {1, {c0}, {3}}, {1, {c0}, {4}}, {1, {c1}, {5}}, {1, {c1}, {6}}};
  if (n == 2) return {{2, {root}, {0, 1}}, {2, {c0}, {2, 3}}, {2, {c0, {1, s.off_w2, 4, s.rb[2], "ACGT"}}, {4, -4, 5}}, {1, {c1}, {6}}};
  return {{7, {root, {2, s.off_w7[0], 3, s.rb[1], "ACG"}, {5, s.off_w7[1], 4, s.rb[2], "ACGT"}}, {0, 1, -3, 2, 3, 4, -4, 5, 6}}};
}
// what a window's destination is in the session: R records, D = min(R, cores + 2) directory entries
struct Taken {
  u64 cap_slice;
  u32 cap_dir;
  std::unique_ptr<u8[]> slice;
  std::unique_ptr<scalce_fq_bucket[]> dir;
  ReadsDst to;
  Taken(int L, u64 R, u32 D) : cap_slice(R * ((u64)(L + 3) / 4 + 2) + 12 * D), cap_dir(D), slice(new u8[cap_slice]), dir(new scalce_fq_bucket[D]),
                               to{slice.get(), dir.get(), cap_slice, cap_dir} {}
  Taken(int L, u64 R) : Taken(L, R, (u32)std::min<u64>(R, 4)) {}
};
static void windows_are_right(const Shape &s, u64 n, Read rd) {
  Arc a(s.L);
  a.r[0].bytes = read_stream(s);
  a.feed(rd, NO_SKIP);
  CHECK(a.open() == SCALCE_OK && a.am[0].L == s.L && a.am[0].no_ac == 0 && !a.w.names && a.w.library == "lib" && a.am[0].phred == 33);
  for (const XWin &x : expected_windows(s, n)) {
    Taken t(s.L, n);
    u64 got = ~0ull;
    CHECK(a.w.reads(0, n, &t.to, got, a.f) == SCALCE_OK && got == x.got && t.to.ndir == x.dir.size());
    for (size_t k = 0; k < x.dir.size(); k++) {
      const scalce_fq_bucket &b = t.dir[k];
      static const char zero[32] = {0};
      CHECK(b.first == x.dir[k].first && b.off == x.dir[k].off && b.core_len == x.dir[k].core_len && b.rec_bytes == x.dir[k].rec_bytes);
      CHECK(!memcmp(b.core, x.dir[k].core, b.core_len) && !memcmp(b.core + b.core_len, zero, sizeof b.core - b.core_len));
    }
    Bytes want;
    for (int seg : x.segs) put(want, seg >= 0 ? record(s, seg) : bucket_header(BUCKETS[-1 - seg].core, BUCKETS[-1 - seg].count));
    CHECK(t.to.bytes == want.size() && !memcmp(t.slice.get(), want.data(), want.size()));
    if (s.L == 5 && n == 7) CHECK(want.size() == sizeof L5_SLICE_OF_ALL && !memcmp(t.slice.get(), L5_SLICE_OF_ALL, sizeof L5_SLICE_OF_ALL));
  }
  Taken t(s.L, n);
  u64 got = ~0ull;
  CHECK(a.w.reads(0, n, &t.to, got, a.f) == SCALCE_OK && got == 0 && t.to.ndir == 0 && t.to.bytes == 0);  // the stream has ended
}

// k records passed over, then the rest taken: what remains is the tail of what taking everything gives
static void pass_over_then_take(const Shape &s, u64 k, Read rd, Skip sk, bool decides) {
  Arc a(s.L);
  a.r[0].bytes = read_stream(s);
  a.feed(rd, sk);
  CHECK(a.open() == SCALCE_OK);
  a.w.known = !decides;  // (no names, no raw qualities: without a symbol count the read stream of the pass's first mate decides)
  CHECK(a.w.decides_count(0, 0) == decides && !a.w.decides_count(0, 3) && !a.w.decides_count(1, 0));
  u64 got = ~0ull, first = k;
  int rc = a.w.reads(0, k, nullptr, got, a.f);
  if (sk == SHORT && k) {  // (one byte per read: the look-ahead buffer never holds a byte of a record, so the first one is skipped)
    FAILED_WITH(rc, a.f, 0, 0, 0, "(ERROR) truncated read stream");
    return;
  }
  CHECK(rc == SCALCE_OK && got == std::min<u64>(k, 7));
  if (sk == EXACT && rd == ONE_BYTE && k) CHECK(a.RS.bytes_skipped[0][0] > 0);
  if (sk == NO_SKIP) CHECK(a.RS.bytes_skipped[0][0] == 0);
  rc = a.w.ended_at(0, 0, got, first, a.f);
  if (k == 8 && !decides) {
    FAILED_WITH(rc, a.f, 0, 0, 0, "(ERROR) truncated read stream");
    return;
  }
  CHECK(rc == SCALCE_OK && first == std::min<u64>(k, 7));  // k = 8, one more than there are: the range is empty, first = 7
  Taken t(s.L, 7);
  CHECK(a.w.reads(0, 7, &t.to, got, a.f) == SCALCE_OK && got == 7 - first);
  u64 seen = 0;
  for (u32 d = 0; d < t.to.ndir; d++) {
    const scalce_fq_bucket &b = t.dir[d];
    const u64 end = d + 1 < t.to.ndir ? t.dir[d + 1].first : got;
    CHECK(b.first == seen);
    for (u64 i = b.first; i < end; i++, seen++) {
      const int rec = (int)(first + i);
      const Bytes want = record(s, rec);
      CHECK(b.rec_bytes == want.size() && b.core_len == rec_core_len(rec) && !memcmp(t.slice.get() + b.off + (i - b.first) * b.rec_bytes, want.data(), want.size()));
    }
  }
  CHECK(seen == got);
}

// ---- mate 2, raw quality rows, length entries ------------------------------------------------------------------------------------
static void mate2_and_rows() {
  for (int pass = 0; pass < 2; pass++) {  // into a destination, and passed over
    Arc a(5);
    a.mates = 2;
    a.r[0].bytes = read_stream(SHAPES[0]);
    put(a.r[1].bytes, Bytes{1, 2, 3, 4, 5, 6, 7});  // bare records of (5 + 3) / 4 = 2 bytes: three of them, and one cut inside
    a.feed(pass ? ONE_BYTE : ODD_PIECES, NO_SKIP);
    CHECK(a.open() == SCALCE_OK);
    Taken two(5, 2, 1), four(5, 4, 1);
    u64 got = ~0ull;
    CHECK(a.w.reads(1, 2, pass ? nullptr : &two.to, got, a.f) == SCALCE_OK && got == 2);
    if (!pass) {
      const scalce_fq_bucket &b = two.dir[0];
      CHECK(two.to.ndir == 1 && two.to.bytes == 4 && b.first == 0 && b.off == 0 && b.core_len == 0 && b.rec_bytes == 2);
      CHECK(!memcmp(two.slice.get(), "\x01\x02\x03\x04", 4));
    }
    FAILED_WITH(a.w.reads(1, 4, pass ? nullptr : &four.to, got, a.f), a.f, 1, 0, 0, "(ERROR) truncated read stream");
  }
  for (int inside = 0; inside < 2; inside++)  // -A: three rows of L = 5 bytes; the stream ends there, or two bytes further on
    for (int pass = 0; pass < 2; pass++) {
      Arc a(5, 1);
      for (u8 v = 1; v <= (inside ? 17 : 15); v++) a.q[0].bytes.push_back(v);
      a.feed(pass ? ODD_PIECES : ONE_BYTE, pass ? EXACT : NO_SKIP);
      CHECK(a.open() == SCALCE_OK && a.am[0].no_ac == 1 && !a.am[0].q_empty && a.w.decides_count(0, 2) && !a.w.decides_count(0, 0));
      std::unique_ptr<u8[]> two(new u8[10]), four(new u8[20]);
      u64 got = ~0ull, n = 4;
      CHECK(a.w.quality_rows(0, 2, pass ? nullptr : two.get(), got, a.f) == SCALCE_OK && got == 2);
      if (!pass) CHECK(!memcmp(two.get(), "\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a", 10));
      const int rc = a.w.quality_rows(0, 4, pass ? nullptr : four.get(), got, a.f);
      if (inside) { FAILED_WITH(rc, a.f, 0, 2, 0, "(ERROR) truncated quality stream"); continue; }
      CHECK(rc == SCALCE_OK && got == 1 && a.w.ended_at(0, 2, got, n, a.f) == SCALCE_OK && n == 1);  // at a row's end: for the caller to judge
      a.w.known = true;
      n = 4;
      FAILED_WITH(a.w.ended_at(0, 2, got, n, a.f), a.f, 0, 2, 0, "(ERROR) truncated quality stream");
    }
  for (int wide = 0; wide < 2; wide++)  // the length stream: entries of one byte (L = 5) and of two (L = 256)
    for (int pass = 0; pass < 2; pass++) {
      const int L = wide ? 256 : 5, width = wide ? 2 : 1;
      Arc a(L);
      a.has_l = true;
      a.l[0].bytes = length_header(width, L);
      for (u8 v = 1; v <= 3 * width; v++) a.l[0].bytes.push_back(v);
      a.feed(pass ? ODD_PIECES : ONE_BYTE, pass ? EXACT : NO_SKIP);
      CHECK(a.open() == SCALCE_OK && a.am[0].has_len && a.am[0].l_width == width);
      std::unique_ptr<u8[]> one(new u8[width]), three(new u8[3 * width]);
      u64 got = ~0ull, n = 3;
      CHECK(a.w.lengths(0, 1, pass ? nullptr : one.get(), got, a.f) == SCALCE_OK && got == 1);
      if (!pass) CHECK(!memcmp(one.get(), "\x01\x02", width));
      CHECK(a.w.lengths(0, 3, pass ? nullptr : three.get(), got, a.f) == SCALCE_OK && got == 2);  // one entry short
      if (!pass) CHECK(!memcmp(three.get(), wide ? "\x03\x04\x05\x06" : "\x02\x03", 2 * width));
      FAILED_WITH(a.w.ended_at(0, 3, got, n, a.f), a.f, 0, 3, 0, "(ERROR) truncated length stream");
    }
  Arc a(256);  // ... and an entry of two bytes cut after its first
  a.has_l = true;
  a.l[0].bytes = length_header(2, 256);
  put(a.l[0].bytes, Bytes{1, 0, 2});
  CHECK(a.open() == SCALCE_OK);
  std::unique_ptr<u8[]> two(new u8[4]);
  u64 got = ~0ull;
  FAILED_WITH(a.w.lengths(0, 2, two.get(), got, a.f), a.f, 0, 3, 0, "(ERROR) truncated length stream");
}

// ---- names ---------------------------------------------------------------------------------------------------------------------------
static Bytes name(size_t len, char c) { Bytes b; b.push_back((u8)len); b.insert(b.end(), len, (u8)c); return b; }
struct NamesTo {
  std::unique_ptr<u8[]> bytes[2];
  std::unique_ptr<u64[]> off[2];
  NamesDst to[2];
  NamesTo(u64 cap, u64 ncap) {
    for (int i = 0; i < 2; i++) { bytes[i].reset(new u8[cap]); off[i].reset(new u64[ncap + 1]); to[i] = NamesDst{bytes[i].get(), off[i].get(), cap}; }
  }
};
static void names() {
  Bytes three = names_header();  // names of 0, 1 and 255 characters: 1 + 2 + 256 bytes
  put(three, name(0, 0)); put(three, name(1, 'a')); put(three, name(255, 'z'));
  for (Read rd : {ONE_BYTE, ODD_PIECES}) {
    for (u64 W : {(u64)1 << 20, (u64)40}) {  // a record of L = 5 counts its name and 2 L + 6 = 16: 16 + 17 fit 40 bytes of text, the third does not
      Arc a(5);
      a.n[0].bytes = three;
      a.feed(rd, NO_SKIP);
      CHECK(a.open() == SCALCE_OK && a.w.names && a.w.rec_budget(0) == 16);
      const u64 want = W == 40 ? 2 : 3;
      NamesTo t(259, 3);
      u64 n = ~0ull, nb[2] = {~0ull, ~0ull};
      CHECK(a.w.take_names(t.to, 3, W, n, nb, a.f) == SCALCE_OK && n == want && nb[0] == (want == 2 ? 3 : 259));
      CHECK(t.off[0][0] == 0 && t.off[0][1] == 1 && t.off[0][2] == 3 && t.off[0][n] == nb[0]);
      CHECK(!memcmp(t.bytes[0].get(), three.data() + 9, nb[0]));
      CHECK(t.bytes[0][0] == 0 && t.bytes[0][1] == 1 && t.bytes[0][2] == 'a' && (n == 2 || (t.bytes[0][3] == 255 && t.bytes[0][258] == 'z')));
      // the name stream decides the count: behind its end a window is empty; with a symbol count it is truncated there
      NamesTo rest(256, 2);
      CHECK(a.w.take_names(rest.to, 2, W, n, nb, a.f) == SCALCE_OK && n == 3 - want);
      CHECK(a.w.take_names(rest.to, 2, W, n, nb, a.f) == SCALCE_OK && n == 0 && nb[0] == 0 && rest.off[0][0] == 0);
      a.w.known = true;
      FAILED_WITH(a.w.take_names(rest.to, 2, W, n, nb, a.f), a.f, 0, 1, 0, "(ERROR) truncated name stream");
    }
    for (u64 k = 0; k <= 4; k++) {  // the hop over k names, then the rest taken
      Arc a(5);
      a.n[0].bytes = three;
      a.feed(rd, k & 1 ? EXACT : NO_SKIP);
      CHECK(a.open() == SCALCE_OK);
      u64 got = ~0ull, n = ~0ull, nb[2];
      CHECK(a.w.pass_names(0, k, got, a.f) == SCALCE_OK && got == std::min<u64>(k, 3) && a.RS.bytes_skipped[0][1] == 0);  // names are always read
      NamesTo t(259, 3);
      CHECK(a.w.take_names(t.to, 3, 1 << 20, n, nb, a.f) == SCALCE_OK && n == 3 - got);
      const size_t at[4] = {0, 1, 3, 259};
      CHECK(nb[0] == 259 - at[got] && !memcmp(t.bytes[0].get(), three.data() + 9 + at[got], nb[0]));
    }
    Arc a(5);  // a name cut after its length byte
    a.n[0].bytes = names_header();
    put(a.n[0].bytes, name(1, 'a')); put(a.n[0].bytes, cut(name(2, 'b'), 1));
    a.feed(rd, NO_SKIP);
    Arc b(5);
    b.n[0].bytes = a.n[0].bytes;
    b.feed(rd, NO_SKIP);
    CHECK(a.open() == SCALCE_OK && b.open() == SCALCE_OK);
    NamesTo t(8, 2);
    u64 n = ~0ull, nb[2], got = ~0ull;
    FAILED_WITH(a.w.take_names(t.to, 2, 1 << 20, n, nb, a.f), a.f, 0, 1, 0, "(ERROR) truncated name stream");
    FAILED_WITH(b.w.pass_names(0, 2, got, b.f), b.f, 0, 1, 0, "(ERROR) truncated name stream");
    Arc p(5);  // two mates in one window; mate 2's names end a record early
    p.mates = 2; p.interleave = 1;
    p.r[0].bytes = read_stream(SHAPES[0]);
    for (int m = 0; m < 2; m++) { p.n[m].bytes = names_header(); put(p.n[m].bytes, name(2, 'p')); }
    put(p.n[0].bytes, name(3, 'q'));
    p.feed(rd, NO_SKIP);
    CHECK(p.open() == SCALCE_OK && p.w.names && p.w.m1 == 1);
    NamesTo pt(7, 2);
    FAILED_WITH(p.w.take_names(pt.to, 2, 1 << 20, n, nb, p.f), p.f, 0, 1, 0, "(ERROR) truncated name stream");
  }
}

// ---- the text-entry streams: comments (stream 5) and plus lines (stream 7), through the functions `scalce -d` walks them with ----
typedef std::vector<std::string> Entries;
static const Read STEPS[3] = {ONE_BYTE, SEVEN_BYTES, EVERYTHING};
struct Noun { int stream; const char *truncated, *too_long, *read_error; };
static const Noun NOUN[2] = {
    {5, "(ERROR) truncated comment stream", "(ERROR) comment stream: an entry is longer than its header says", "read error on the comment stream"},
    {7, "(ERROR) truncated plus-line stream", "(ERROR) plus-line stream: an entry is longer than its header says", "read error on the plus-line stream"}};
// the stream of `entries` (longest: what its header says instead of the truth); a plus-line stream of empty entries is its header
static Bytes text_stream(bool plus, const Entries &entries, int64_t longest = -1) {
  uint32_t c = 0;
  for (const std::string &e : entries) c = std::max<uint32_t>(c, (uint32_t)e.size());
  Bytes out(COMMENT_HEADER_BYTES);
  (plus ? plus_header_write : comment_header_write)(out.data(), longest < 0 ? c : (uint32_t)longest, entries.size());
  if (plus && !c && longest <= 0) return out;
  for (const std::string &e : entries) { put(out, e.c_str()); out.push_back('\n'); }
  return out;
}
static std::string body_of(const Entries &entries, size_t first, size_t n) {
  std::string s;
  for (size_t i = first; i < first + n; i++) s += entries[i] + "\n";
  return s;
}
static Bytes names_of(size_t n) {  // n names of two characters: 3 bytes each, 2 + 16 bytes of a window of reads of 5 bases
  Bytes b = names_header();
  for (size_t i = 0; i < n; i++) put(b, name(2, (char)('a' + i % 26)));
  return b;
}
// an archive of one mate (or an interleaved pair) with a stream of the kind per mate, opened
struct TextArc : Arc {
  bool plus;
  TextArc(bool plus_, Read rd, size_t names, const Bytes &m1, const Bytes *m2 = nullptr) : Arc(5), plus(plus_) {
    (plus ? has_p : has_c) = true;
    if (m2) { mates = 2; interleave = 1; text_feed(plus, 1).bytes = *m2; }
    for (int m = 0; m < mates; m++) n[m].bytes = names_of(names);
    text_feed(plus).bytes = m1;
    feed(rd, NO_SKIP);
  }
  // up to ncap records' (pairs') names and entries, as a window takes them: the entries into a block of exactly `cap` bytes
  std::unique_ptr<u8[]> got;
  u64 nbytes = 0, grow = 0;
  int take(u64 ncap, u64 cap, u64 &cnt, u64 W = (u64)1 << 40) {
    got.reset(new u8[cap ? cap : 1]);
    NamesTo t(3 * ncap, ncap);
    CommentsDst cd{got.get(), cap};
    PlusDst pd{got.get(), cap};
    u64 nb[2];
    const int rc = w.take_names(t.to, ncap, W, cnt, nb, f, plus ? nullptr : &cd, plus ? &pd : nullptr);
    nbytes = plus ? pd.nbytes : cd.nbytes;
    grow = pd.grow;
    return rc;
  }
  std::string taken() const { return std::string(got.get(), got.get() + nbytes); }
};

// every entry of a stream in groups of 1, 2 and all, alternately taken with the records' names and passed over, at every
// delivery step.  (The cursors this walk replaced were also run with buffers of 1, 5 and 64 bytes, to break entries across
// refills.  Src has one look-ahead buffer of 1 MiB that grows, so that dimension has no counterpart here: an entry spans
// refills when it arrives in steps of 1 and 7 bytes, and the entries of 65535 bytes are the longest a stream may hold.)
static void text_walks(bool plus, const Entries &entries) {
  const Noun &noun = NOUN[plus];
  const Bytes data = text_stream(plus, entries);
  const size_t N = entries.size();
  uint32_t longest = 0;
  for (const std::string &e : entries) longest = std::max<uint32_t>(longest, (uint32_t)e.size());
  for (Read rd : STEPS)
    for (size_t group : {(size_t)1, (size_t)2, N ? N : (size_t)1}) {
      TextArc a(plus, rd, N + 1, data);
      CHECK(a.open() == SCALCE_OK);
      TextStream &t = a.text(plus);
      CHECK(t.open && t.total == N && t.longest == longest && t.taken == 0 && t.kind->stream == noun.stream);
      std::string want;
      bool skipping = false;
      for (size_t k = 0; k < N; skipping = !skipping) {
        const size_t n = std::min(group, N - k);
        u64 got = ~0ull;
        if (skipping) {
          CHECK(a.w.pass_text(0, t, n, got, a.f) == SCALCE_OK && got == n);
          CHECK(a.w.pass_names(0, n, got, a.f) == SCALCE_OK && got == n);
        } else {
          want = body_of(entries, k, n);
          CHECK(a.take(n, want.size(), got) == SCALCE_OK && got == n && a.taken() == want);  // the entries with their newlines
        }
        k += n;
        CHECK(t.taken == k);
      }
      u64 got = ~0ull;
      CHECK(a.w.pass_text(0, t, 1, got, a.f) == SCALCE_OK && got == 0);  // it ends here, between two entries ...
      FAILED_WITH(a.take(1, 1, got), a.f, 0, noun.stream, 0, noun.truncated);  // ... where a record that has a name wants one more
      CHECK(t.taken == N && t.delivered == data.size() && t.skipped == 0);
      // what the session says when the archive holds another count: up front from the header's, at the end from what was taken
      const std::string held = std::string(plus ? "(ERROR) plus-line" : "(ERROR) comment") + " stream holds " + std::to_string(N) + " entries, the archive ";
      FAILED_WITH(a.w.text_count(0, t, t.total, N + 1, a.f), a.f, 0, noun.stream, 0, (held + std::to_string(N + 1) + " records").c_str());
      FAILED_WITH(a.w.text_count(0, t, t.total, t.taken, a.f), a.f, 0, noun.stream, 0, (held + std::to_string(N) + " records").c_str());
    }
}

// a stream of three entries cut at every byte: inside the header the open fails; behind it exactly the entries whose newline
// survived are given, then the stream is truncated (the cut lies inside an entry) or ends there (between two)
static void text_cuts(bool plus, const Entries &entries) {
  const Noun &noun = NOUN[plus];
  const Bytes whole = text_stream(plus, entries);
  std::vector<size_t> ends;  // where each entry's newline lies
  for (size_t i = COMMENT_HEADER_BYTES; i < whole.size(); i++)
    if (whole[i] == '\n') ends.push_back(i);
  CHECK(ends.size() == 3 && entries.size() == 3);
  for (size_t at = 0; at < whole.size(); at++)
    for (Read rd : STEPS) {
      TextArc a(plus, rd, 3, cut(whole, at));
      const int rc = a.open();
      if (at < COMMENT_HEADER_BYTES) { FAILED_WITH(rc, a.f, 0, noun.stream, 0, noun.truncated); continue; }
      TextStream &t = a.text(plus);
      CHECK(rc == SCALCE_OK && t.total == 3 && t.longest == (plus ? 3u : 13u));
      size_t complete = 0;
      for (size_t e : ends) complete += e < at ? 1 : 0;
      for (size_t k = 0; k < complete; k++) {
        u64 got = ~0ull;
        const std::string want = entries[k] + "\n";
        if (k & 1) CHECK(a.w.pass_text(0, t, 1, got, a.f) == SCALCE_OK && got == 1 && a.w.pass_names(0, 1, got, a.f) == SCALCE_OK);
        else CHECK(a.take(1, want.size(), got) == SCALCE_OK && got == 1 && a.taken() == want);
      }
      const size_t begins = complete ? ends[complete - 1] + 1 : COMMENT_HEADER_BYTES;  // the first entry that is not whole
      const u8 *p = nullptr;
      size_t len = 0;
      u64 got = ~0ull;
      if (at > begins) {
        FAILED_WITH(a.w.next_text(0, t, p, len, a.f), a.f, 0, noun.stream, 0, noun.truncated);
        FAILED_WITH(a.w.pass_text(0, t, 3, got, a.f), a.f, 0, noun.stream, 0, noun.truncated);
      } else {
        CHECK(a.w.next_text(0, t, p, len, a.f) == 1);
        CHECK(a.w.pass_text(0, t, 3, got, a.f) == SCALCE_OK && got == 0);
      }
      CHECK(t.taken == complete);
    }
}

// an entry longer than the header says fails whether its newline is in the buffer or not yet; one of exactly that length passes
static void text_length_edges(bool plus, const Entries &entries, uint32_t too_short) {
  const Noun &noun = NOUN[plus];
  for (Read rd : STEPS) {
    TextArc a(plus, rd, 3, text_stream(plus, entries, too_short));  // the second entry holds one byte more
    CHECK(a.open() == SCALCE_OK && a.text(plus).longest == too_short && entries[1].size() == too_short + 1);
    u64 got = ~0ull;
    const std::string first = entries[0] + "\n";
    CHECK(a.take(1, first.size(), got) == SCALCE_OK && got == 1 && a.taken() == first);
    Failure passed;
    FAILED_WITH(a.w.pass_text(0, a.text(plus), 2, got, passed), passed, 0, noun.stream, 0, noun.too_long);
    FAILED_WITH(a.take(2, 64, got), a.f, 0, noun.stream, 0, noun.too_long);
    TextArc b(plus, rd, 3, text_stream(plus, entries, too_short + 1));
    CHECK(b.open() == SCALCE_OK && b.w.pass_text(0, b.text(plus), 3, got, b.f) == SCALCE_OK && got == 3 && b.text(plus).taken == 3);
  }
}

// a read callback that fails at its first, its second and a later call (one byte per call): in the header twice, then inside
// the first entry -- what `scalce -d` says of a file it cannot read
static void text_failed_read(bool plus, const Entries &entries) {
  const Noun &noun = NOUN[plus];
  for (int call : {0, 1, (int)COMMENT_HEADER_BYTES + 1})
    for (int taking = 0; taking < 2; taking++) {
      TextArc a(plus, ONE_BYTE, 2, text_stream(plus, entries));
      a.text_feed(plus).error_call = call;
      const int rc = a.open();
      if (call < (int)COMMENT_HEADER_BYTES) { FAILED_WITH(rc, a.f, 0, noun.stream, 0, noun.read_error); continue; }
      u64 got = ~0ull;
      CHECK(rc == SCALCE_OK);
      FAILED_WITH(taking ? a.take(2, 64, got) : a.w.pass_text(0, a.text(plus), 2, got, a.f), a.f, 0, noun.stream, 0, noun.read_error);
    }
  const Bytes good = text_stream(plus, entries);  // ... and on mate 2's stream, inside its second entry
  TextArc p(plus, ONE_BYTE, 2, good, &good);
  p.text_feed(plus, 1).error_call = (int)(COMMENT_HEADER_BYTES + entries[0].size() + 2);
  u64 got = ~0ull;
  CHECK(p.open() == SCALCE_OK);
  FAILED_WITH(p.take(2, 64, got), p.f, 1, noun.stream, 0, noun.read_error);
}

// what only take_names does with the entries: two mates in one window, a budget and a destination that an entry fills, and
// mate 2's stream ending before mate 1's
static void text_windows(bool plus) {
  const Noun &noun = NOUN[plus];
  u64 got = ~0ull;
  {  // a pair's entries land as mate 1's then mate 2's, pair by pair
    const Entries m1 = plus ? Entries{"=", "", "'x"} : Entries{" a1", "", " a3"}, m2 = plus ? Entries{"", "'yz", "="} : Entries{" b1", " b22", ""};
    const Bytes s2 = text_stream(plus, m2);
    std::string want;
    for (size_t k = 0; k < 3; k++) want += m1[k] + "\n" + m2[k] + "\n";
    for (Read rd : STEPS) {
      TextArc a(plus, rd, 3, text_stream(plus, m1), &s2);
      CHECK(a.open() == SCALCE_OK && a.w.m1 == 1);
      CHECK(a.take(3, want.size(), got) == SCALCE_OK && got == 3 && a.taken() == want && a.text(plus, 0).taken == 3 && a.text(plus, 1).taken == 3);
      if (plus) CHECK(a.grow == 2 + 0 + 0 + 2 + 1 + 2);  // (a repeat adds the name's 2 bytes, a literal its bytes behind the class byte)
    }
  }
  {  // a record is its name and 2 L + 6 = 18 bytes of text, and what its entry adds: 7 bytes in the second record here
    const Entries e = plus ? Entries{"", "'bcdefgh", ""} : Entries{"", " bcdefg", ""};
    for (u64 W : {(u64)18 + 25 - 1, (u64)18 + 25}) {  // the second record's 25 bytes push the window over W, or just fit
      TextArc a(plus, ODD_PIECES, 3, text_stream(plus, e)), bare(plus, ODD_PIECES, 3, text_stream(plus, e));
      CHECK(a.open() == SCALCE_OK && bare.open() == SCALCE_OK);
      const u64 fits = W == 42 ? 1 : 2;
      CHECK(a.take(2, 64, got, W) == SCALCE_OK && got == fits && a.taken() == body_of(e, 0, fits) && a.text(plus).taken == fits);
      NamesTo t(6, 2);  // (the names alone: two records of 18 bytes fit either window -- the entry ends it one record sooner)
      u64 nb[2];
      CHECK(bare.w.take_names(t.to, 2, W, got, nb, bare.f) == SCALCE_OK && got == 2);
    }
  }
  {  // a destination whose cap the second record's entry reaches: the window ends in front of it, and nothing of it is taken
    const Entries e = plus ? Entries{"=", "=", "="} : Entries{" ", " ", " "};
    for (u64 cap : {(u64)3, (u64)4}) {
      TextArc a(plus, ODD_PIECES, 3, text_stream(plus, e));
      CHECK(a.open() == SCALCE_OK);
      const u64 fits = cap / 2;
      CHECK(a.take(3, cap, got) == SCALCE_OK && got == fits && a.nbytes == 2 * fits && a.taken() == body_of(e, 0, fits) && a.text(plus).taken == fits);
    }
  }
  {  // mate 2's stream ends between two entries while mate 1's goes on: truncated, on mate 2
    const Entries m1 = plus ? Entries{"=", "'x"} : Entries{" a", " b"}, m2 = plus ? Entries{"="} : Entries{" c"};
    const Bytes s2 = text_stream(plus, m2);
    TextArc a(plus, ODD_PIECES, 2, text_stream(plus, m1), &s2);
    CHECK(a.open() == SCALCE_OK);
    FAILED_WITH(a.take(2, 64, got), a.f, 1, noun.stream, 0, noun.truncated);
  }
}

// what the plus-line stream alone has
static void plus_lines() {
  {  // P = 0: the file is its header.  Nothing is read behind it; N bare entries, then the stream ends
    const Bytes data = text_stream(true, {"", "", "", ""});
    CHECK(data.size() == PLUS_HEADER_BYTES);
    TextArc a(true, EVERYTHING, 4, data);
    CHECK(a.open() == SCALCE_OK && a.am[0].plus.longest == 0 && a.am[0].plus.total == 4 && a.am[0].plus.no_entries());
    const int calls = a.p[0].calls;
    u64 got = ~0ull;
    CHECK(a.w.pass_text(0, a.am[0].plus, 1, got, a.f) == SCALCE_OK && got == 1);
    for (int k = 1; k < 4; k++) {
      const u8 *at = nullptr;
      size_t len = 0;
      PlusClass cls = PLUS_MALFORMED;
      CHECK(a.w.next_plus(0, at, len, cls, a.f) == 0 && len == 1 && at[0] == '\n' && cls == PLUS_BARE);
      a.w.text_taken(a.am[0].plus, len);
    }
    const u8 *at = nullptr;
    size_t len = 0;
    PlusClass cls = PLUS_MALFORMED;
    CHECK(a.w.next_plus(0, at, len, cls, a.f) == 1 && a.am[0].plus.taken == 4);
    CHECK(a.w.pass_text(0, a.am[0].plus, 2, got, a.f) == SCALCE_OK && got == 0);
    CHECK(a.p[0].calls == calls && a.am[0].plus.delivered == PLUS_HEADER_BYTES);
  }
  {  // every class, as next_plus names it
    const Entries e = {"", "=", "'a", "'=", "''", "'= x"};
    const PlusClass want[6] = {PLUS_BARE, PLUS_REPEAT, PLUS_LITERAL, PLUS_LITERAL, PLUS_LITERAL, PLUS_LITERAL};
    for (Read rd : STEPS) {
      TextArc a(true, rd, 6, text_stream(true, e));
      CHECK(a.open() == SCALCE_OK);
      for (size_t k = 0; k < 6; k++) {
        const u8 *at = nullptr;
        size_t len = 0;
        PlusClass cls = PLUS_MALFORMED;
        CHECK(a.w.next_plus(0, at, len, cls, a.f) == 0 && cls == want[k] && std::string(at, at + len) == e[k] + "\n");
        a.w.text_taken(a.am[0].plus, len);
      }
    }
  }
  // ... and the entries that are of none: '=' with more behind it, a literal of nothing (it would be the bare line), another first byte
  for (const char *bad : {"=x", "=a", "==", "'", "x", "a", "+r1", "+a", " "})
    for (Read rd : STEPS) {
      TextArc a(true, rd, 3, text_stream(true, {"=", bad, ""}, 8));
      CHECK(a.open() == SCALCE_OK);
      const u8 *at = nullptr;
      size_t len = 0;
      PlusClass cls = PLUS_MALFORMED;
      u64 got = ~0ull;
      CHECK(a.w.next_plus(0, at, len, cls, a.f) == 0 && cls == PLUS_REPEAT);
      a.w.text_taken(a.am[0].plus, len);
      Failure peeked;
      FAILED_WITH(a.w.next_plus(0, at, len, cls, peeked), peeked, 0, 7, 0, "(ERROR) plus-line stream: malformed entry");
      FAILED_WITH(a.w.pass_text(0, a.am[0].plus, 2, got, a.f), a.f, 0, 7, 0, "(ERROR) plus-line stream: malformed entry");
    }
  {  // what an entry adds to its record, through plus_peek: header = the header line behind '@', here a name of 10 bytes and a
     // comment of 7.  A repeat grows the record by both, a literal by its bytes behind the class byte, a bare line by nothing
    TextArc a(true, SEVEN_BYTES, 3, text_stream(true, {"=", "'abcd", ""}));
    CHECK(a.open() == SCALCE_OK);
    const u64 header[2] = {10 + 7, 0}, grows[3] = {17, 4, 0};
    std::unique_ptr<u8[]> to(new u8[9]);
    PlusDst pd{to.get(), 9}, small{to.get(), 1};
    for (int k = 0; k < 3; k++) {
      Walk::PlusPeek pk;
      CHECK(a.w.plus_peek(header, pk, a.f) == SCALCE_OK && pk.grow == grows[k] && a.am[0].plus.taken == (u64)k);  // (nothing is consumed yet)
      CHECK(a.w.plus_fits(pd, pk) && a.w.plus_fits(small, pk) == (k == 2));
      a.w.plus_commit(pd, pk);
    }
    Walk::PlusPeek pk;
    CHECK(a.w.plus_peek(header, pk, a.f) == 1);
    CHECK(pd.nbytes == 9 && !memcmp(to.get(), "=\n'abcd\n\n", 9) && pd.grow == 21);
  }
  {  // ... and as a window counts it: the comment that take_names puts behind the name is part of what a repeat repeats
    Arc a(5);
    a.has_c = a.has_p = true;
    a.n[0].bytes = names_of(1);
    a.c[0].bytes = text_stream(false, {" xyz"});
    a.p[0].bytes = text_stream(true, {"="});
    CHECK(a.open() == SCALCE_OK);
    NamesTo t(3, 1);
    std::unique_ptr<u8[]> cb(new u8[5]), pb(new u8[2]);
    CommentsDst cd{cb.get(), 5};
    PlusDst pd{pb.get(), 2};
    u64 n = ~0ull, nb[2];
    CHECK(a.w.take_names(t.to, 1, 1 << 20, n, nb, a.f, &cd, &pd) == SCALCE_OK && n == 1);
    CHECK(cd.nbytes == 5 && !memcmp(cb.get(), " xyz\n", 5) && pd.nbytes == 2 && !memcmp(pb.get(), "=\n", 2) && pd.grow == 2 + 4);
  }
}

static void text_streams() {
  for (int plus = 0; plus < 2; plus++) {
    const std::vector<Entries> sets = plus ? std::vector<Entries>{{}, {""}, {"="}, {"=", "", "'SRR001666.1 length=36", "'=", "", "=", "''x"},
                                                                  {"'" + std::string(65534, 'q'), "", "=", "'" + std::string(65534, ' ')}}
                                           : std::vector<Entries>{{}, {""}, {" "}, {"", " ", " 1:N:0:ATCACG", "", " length=100"},
                                                                  {std::string(65535, 'q'), "", "x", std::string(65535, ' ')}};
    for (const Entries &e : sets) text_walks(plus, e);
    text_cuts(plus, plus ? Entries{"'ab", "", "="} : Entries{" 1:N:0:ATCACG", "", " "});
    text_length_edges(plus, plus ? Entries{"=", "'abc", ""} : Entries{" ab", " abcd", " a"}, plus ? 3 : 4);
    text_failed_read(plus, plus ? Entries{"=", "'a"} : Entries{" x", " y"});
    text_windows(plus);
  }
  plus_lines();
}

// ---- the hop over coded frames ---------------------------------------------------------------------------------------------------
static void frames() {
  Bytes all = quality_header();  // (behind the header the session takes the table and the symbol count; the hop begins at a size word)
  const uint32_t sizes[3] = {5, 7, 300};
  for (uint32_t sz : sizes) { put(all, sz); all.insert(all.end(), sz, (u8)sz); }
  put(all, (u8)9);
  const size_t second = 16 + 4 + 5;  // where the second frame's size word begins
  for (Read rd : {ONE_BYTE, ODD_PIECES})
    for (Skip sk : {NO_SKIP, EXACT}) {
      Arc a(5);
      a.q[0].bytes = all;
      a.feed(rd, sk);
      CHECK(a.open() == SCALCE_OK && a.w.pass_frames(0, 3, a.f) == SCALCE_OK);
      CHECK(a.am[0].q.need(1) && a.am[0].q.ptr()[0] == 9 && !a.am[0].q.need(2));  // what follows the third frame is next
      if (sk == EXACT && rd == ONE_BYTE) CHECK(a.RS.bytes_skipped[0][2] == 5 + 7 + 300);  // no read ahead of a size word
      for (size_t at : {second + 2, second + 4 + 3}) {  // cut inside the second frame's size word, and inside its bytes
        Arc c(5);
        c.q[0].bytes = cut(all, at);
        c.feed(rd, sk);
        CHECK(c.open() == SCALCE_OK);
        FAILED_WITH(c.w.pass_frames(0, 3, c.f), c.f, 0, 2, 0, "(ERROR) truncated quality stream");
      }
    }
  u64 pl[4];  // the plan in front of the hop: frames of SCALCE_AC_BLOCK symbols, records of 100
  CHECK(range_plan_quality(0, 0, 1, 100, pl) == SCALCE_ERR_ARG);
  CHECK(range_plan_quality(100, 0, ~0ull, 2 * FRAME + 50, pl) == SCALCE_OK && pl[0] == 0 && pl[1] == 3 && pl[2] == 0 && pl[3] == 2 * FRAME + 50);
  // (record 104858 begins at symbol 10485800, 40 symbols into the second frame of 10485760)
  CHECK(range_plan_quality(100, 104858, 1, 2 * FRAME + 50, pl) == SCALCE_OK && pl[0] == 1 && pl[1] == 1 && pl[2] == 40 && pl[3] == 100);
  // (behind the end: clamped to the 209715 whole records, whose end, symbol 20971500, lies in the second frame)
  CHECK(range_plan_quality(100, ~0ull, 5, 2 * FRAME + 50, pl) == SCALCE_OK && pl[0] == 1 && pl[1] == 0 && pl[2] == 0 && pl[3] == 0);
}

// ---- malformed headers, failing callbacks ------------------------------------------------------------------------------------------
static Bytes one_bucket(int L, int32_t core) { Bytes b = reads_header(L); put(b, bucket_header(core, 1)); put(b, Bytes(8, 0)); return b; }
static void malformed() {
  {
    Arc a(5);
    a.r[0].bytes[3] = 'x';
    FAILED_WITH(a.open(), a.f, 0, 0, 1, "is not a scalce archive");
    Arc b(0), c(-1);
    FAILED_WITH(b.open(), b.f, 0, 0, 0, "(ERROR) read length 0 in the read stream's header");
    FAILED_WITH(c.open(), c.f, 0, 0, 0, "(ERROR) read length -1 in the read stream's header");
    Arc d(5);  // the second mate's header is looked at as well
    d.mates = 2;
    d.r[1].bytes = cut(reads_header(5), 10);
    FAILED_WITH(d.open(), d.f, 1, 0, 0, "(ERROR) truncated read stream");
    Arc e(5);  // a length stream written for another read length
    e.has_l = true;
    e.l[0].bytes = length_header(1, 6);
    FAILED_WITH(e.open(), e.f, 0, 3, 0, "(ERROR) the length stream was written for reads of up to 6 bases, the read stream holds reads of 5");
    Arc g(5);
    g.has_l = true;
    g.l[0].bytes = cut(length_header(1, 5), 15);
    FAILED_WITH(g.open(), g.f, 0, 3, 0, "(ERROR) truncated length stream");
  }
  const struct { int L; int32_t core; const char *msg; } bad_core[4] = {
      {5, 2, "(ERROR) archive refers to core 2 which the core table does not have"},   // the count itself
      {5, -2, "(ERROR) archive refers to core -2 which the core table does not have"},
      {3, 1, "(ERROR) core 1 does not fit the reads"},                                 // four bases of core in a read of three
      {3, 0, nullptr}};                                                                // (three do fit)
  for (const auto &c : bad_core)
    for (int pass = 0; pass < 2; pass++) {
      Arc a(c.L);
      a.r[0].bytes = one_bucket(c.L, c.core);
      CHECK(a.open() == SCALCE_OK);
      Taken t(c.L, 1);
      u64 got = ~0ull;
      const int rc = a.w.reads(0, 1, pass ? nullptr : &t.to, got, a.f);
      if (c.msg) FAILED_WITH(rc, a.f, 0, 0, 0, c.msg);
      else CHECK(rc == SCALCE_OK && got == 1);
    }
  for (size_t have = 1; have <= 11; have++)  // a bucket header cut after each of its first 11 bytes ends the stream: no error
    for (int err = 0; err < 2; err++) {      // ... unless the callback failed
      Arc a(5);
      a.r[0].bytes = cut(one_bucket(5, 0), 16 + have);
      a.feed(ONE_BYTE, NO_SKIP);
      if (err) a.r[0].error_call = 16 + (int)have;  // (one byte per call: the call behind the last byte there is)
      CHECK(a.open() == SCALCE_OK);
      bool more = true;
      const int rc = a.w.more_reads(0, 1, more, a.f);
      if (err) FAILED_WITH(rc, a.f, 0, 0, 0, "read error on the read stream");
      else CHECK(rc == SCALCE_OK && !more && a.w.next_bucket(0, a.f) == 1);
    }
  {
    Arc a(5);  // more buckets than the directory has entries: five of one record each in a window of five, D = min(5, 2 + 2)
    const int32_t cores[5] = {SCALCE_ROOT_CORE, 0, 1, 0, 1};
    for (int32_t c : cores) { put(a.r[0].bytes, bucket_header(c, 1)); put(a.r[0].bytes, Bytes(c == SCALCE_ROOT_CORE ? 3 : 2, 0x55)); }
    CHECK(a.open() == SCALCE_OK);
    Taken t(5, 5);
    u64 got = ~0ull;
    FAILED_WITH(a.w.reads(0, 5, &t.to, got, a.f), a.f, 0, 0, 0, "(ERROR) the read stream opens more buckets than the core table has cores");
    CHECK(t.to.ndir == 4);
  }
  {
    Arc a(5);  // what check_end asks: a range that ends with the archive, and a read stream that holds one record more
    a.r[0].bytes = one_bucket(5, 0);
    a.feed(ONE_BYTE, NO_SKIP);
    CHECK(a.open() == SCALCE_OK);
    int more = -2;
    a.am[0].range_left = 0;  // (a range that ends sooner: nothing behind it is read)
    CHECK(a.w.reads_at_end(more, a.f) == SCALCE_OK && more == -1 && a.RS.bytes_delivered[0][0] == 16);
    a.am[0].range_left = UNKNOWN;
    a.am[0].first = 12;
    CHECK(a.w.reads_at_end(more, a.f) == SCALCE_OK && more == 0);
    FAILED_WITH(a.w.holds_more(0, a.f), a.f, 0, 0, 0, "(ERROR) the read stream holds more than the 12 records of the quality stream");
  }
  // a read callback that fails at its k-th call (one byte per call, so k is the byte it fails in front of), stream by stream
  const struct { int k; const char *msg; int wants_file; } r_fails[3] = {
      {3, "is not a scalce archive", 1}, {9, "(ERROR) truncated read stream", 0}, {14, "(ERROR) truncated read stream", 0}};
  for (const auto &c : r_fails) {
    Arc a(5);
    a.feed(ONE_BYTE, NO_SKIP);
    a.r[0].error_call = c.k;
    FAILED_WITH(a.open(), a.f, 0, 0, c.wants_file, c.msg);
  }
  for (int k : {16 + 12 + 1, 16 + 12 + 3 + 12 + 12 + 1})  // inside a record of the root bucket, and of the bucket behind the empty one
    for (int pass = 0; pass < 2; pass++) {
      Arc a(5);
      a.r[0].bytes = read_stream(SHAPES[0]);
      a.feed(ONE_BYTE, NO_SKIP);
      a.r[0].error_call = k;
      CHECK(a.open() == SCALCE_OK);
      Taken t(5, 7);
      u64 got = ~0ull;
      FAILED_WITH(a.w.reads(0, 7, pass ? nullptr : &t.to, got, a.f), a.f, 0, 0, 0, "read error on the read stream");
    }
  for (int k : {0, 15, 16}) {  // the quality stream: inside its header, and at the byte that says whether it holds anything
    Arc a(5, 1);
    put(a.q[0].bytes, Bytes(10, 1));
    a.feed(ONE_BYTE, NO_SKIP);
    a.q[0].error_call = k;
    FAILED_WITH(a.open(), a.f, 0, 2, 0, "read error on the quality stream");
  }
  for (int pass = 0; pass < 2; pass++) {  // ... and inside its rows
    Arc a(5, 1);
    put(a.q[0].bytes, Bytes(10, 1));
    a.feed(ONE_BYTE, NO_SKIP);
    a.q[0].error_call = 16 + 7;
    CHECK(a.open() == SCALCE_OK);
    std::unique_ptr<u8[]> two(new u8[10]);
    u64 got = ~0ull;
    FAILED_WITH(a.w.quality_rows(0, 2, pass ? nullptr : two.get(), got, a.f), a.f, 0, 2, 0, "read error on the quality stream");
  }
  for (int pass = 0; pass < 2; pass++) {  // the name stream: in front of a name's length byte
    Arc a(5);
    a.n[0].bytes = names_header();
    put(a.n[0].bytes, name(1, 'a')); put(a.n[0].bytes, name(1, 'b'));
    a.feed(ONE_BYTE, NO_SKIP);
    a.n[0].error_call = 9 + 2;
    CHECK(a.open() == SCALCE_OK);
    NamesTo t(4, 2);
    u64 n = ~0ull, nb[2], got = ~0ull;
    FAILED_WITH(pass ? a.w.pass_names(0, 2, got, a.f) : a.w.take_names(t.to, 2, 1 << 20, n, nb, a.f), a.f, 0, 1, 0, "read error on the name stream");
  }
  for (int k : {5, 16 + 1}) {  // the length stream: inside its header, inside its entries
    Arc a(5);
    a.has_l = true;
    a.l[0].bytes = length_header(1, 5);
    put(a.l[0].bytes, Bytes{0, 1, 2});
    a.feed(ONE_BYTE, NO_SKIP);
    a.l[0].error_call = k;
    const int rc = a.open();
    std::unique_ptr<u8[]> three(new u8[3]);
    u64 got = ~0ull;
    FAILED_WITH(k < 16 ? rc : a.w.lengths(0, 3, three.get(), got, a.f), a.f, 0, 3, 0, "read error on the length stream");
  }
  for (int k : {16 + 2, 16 + 4 + 2}) {  // the coded frames: inside a size word, inside a frame
    Arc a(5);
    put(a.q[0].bytes, (uint32_t)6); put(a.q[0].bytes, Bytes(6, 1));
    a.feed(ONE_BYTE, NO_SKIP);
    a.q[0].error_call = k;
    CHECK(a.open() == SCALCE_OK);
    FAILED_WITH(a.w.pass_frames(0, 1, a.f), a.f, 0, 2, 0, "read error on the quality stream");
  }
}

int main() {
  CHECK(read_stream(SHAPES[0]) == Bytes(L5_STREAM, L5_STREAM + sizeof L5_STREAM));
  for (const Shape &s : SHAPES)
    for (Read rd : {ONE_BYTE, ODD_PIECES}) {
      for (u64 n : {1, 2, 7}) windows_are_right(s, n, rd);
      for (u64 k = 0; k <= 8; k++)
        for (int decides = 0; decides < 2; decides++) {
          pass_over_then_take(s, k, rd, NO_SKIP, decides);
          pass_over_then_take(s, k, rd, EXACT, decides);
          if (rd == ONE_BYTE) pass_over_then_take(s, k, rd, SHORT, decides);
        }
    }
  mate2_and_rows();
  names();
  text_streams();
  frames();
  malformed();
  puts("archive_walk_check: ok");
  return 0;
}
