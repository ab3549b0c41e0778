// digeststream_check.cpp -- the host side of the digest stream (scalce_amd/csrc/digeststream.hpp: the .scalced layout, every
// malformed or truncated form with its message, the messages of the check, and the arithmetic that joins CRCs of pieces against
// zlib's crc32_combine64 and crc32) on its own: a program for AddressSanitizer and UBSan, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/digeststream_check.cpp -o /tmp/dc -lz && /tmp/dc
// Every array handed to the code under test is a heap block of exactly the size it may touch.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../scalce_amd/csrc/digeststream.hpp"

using namespace scalce_host;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

static Digest sample(int kind, int texts) {
  Digest d;
  d.kind = kind;
  d.texts = texts;
  d.text[0].bytes = 0x0000000123456789ull;
  d.text[0].crc = 0xCBF43926u;
  d.text[1].bytes = 77;
  d.text[1].crc = 0x00000001u;
  return d;
}
static std::unique_ptr<uint8_t[]> exact(const uint8_t *src, size_t n) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
  memcpy(p.get(), src, n);
  return p;
}

static void round_trip() {
  for (int kind : {0, 1, 2, 4, 5, 6})
    for (int texts : {1, 2}) {
      const Digest d = sample(kind, texts);
      uint8_t buf[DIGEST_MAX_BYTES];
      const size_t n = digest_write(buf, d);
      CHECK(n == 24 + 16 * (size_t)texts);
      CHECK(!memcmp(buf, "scalce22", 8));
      int32_t f[2];
      int64_t t;
      memcpy(f, buf + 8, 8);
      memcpy(&t, buf + 16, 8);
      CHECK(f[0] == 16 && f[1] == kind && t == texts);
      uint64_t by;
      uint32_t w[2];
      memcpy(&by, buf + 24, 8);
      memcpy(w, buf + 32, 8);
      CHECK(by == 0x0000000123456789ull && w[0] == 0xCBF43926u && w[1] == 0);
      auto e = exact(buf, n);
      Digest back;
      CHECK(digest_read(e.get(), n, &back) == nullptr);
      CHECK(back.kind == kind && back.texts == texts);
      for (int i = 0; i < texts; i++) CHECK(back.text[i].bytes == d.text[i].bytes && back.text[i].crc == d.text[i].crc);
    }
  CHECK(digest_kind_texts(0) == 1 && digest_kind_texts(1) == 2 && digest_kind_texts(2) == 1);
  CHECK(digest_kind_texts(4) == 1 && digest_kind_texts(5) == 2 && digest_kind_texts(6) == 1);
}

static void malformed() {
  for (int texts : {1, 2}) {
    uint8_t buf[DIGEST_MAX_BYTES];
    const size_t n = digest_write(buf, sample(1, texts));
    Digest d = sample(0, 1);
    for (size_t have = 0; have < n; have++) {  // cut anywhere
      auto e = exact(buf, have);
      const char *why = digest_read(e.get(), have, &d);
      CHECK(why && !strcmp(why, "truncated digest stream"));
    }
    CHECK(d.kind == 0 && d.texts == 1);  // (nothing filled in on the way)
    auto refused = [&](size_t at, uint8_t v) {
      auto e = exact(buf, n);
      e[at] = v;
      Digest x;
      const char *why = digest_read(e.get(), n, &x);
      return why && !strcmp(why, "is not a scalce digest stream");
    };
    CHECK(refused(0, 'x'));        // the magic
    CHECK(refused(6, '3'));
    CHECK(!refused(7, '3'));       // (the last magic byte is the minor version, as for the other streams)
    CHECK(refused(8, 8));          // an entry width that is not 16
    CHECK(refused(12, 3));         // kinds that do not exist
    CHECK(refused(12, 7));
    CHECK(refused(12, 8));
    CHECK(refused(15, 0x80));
    CHECK(refused(16, 0));         // no texts, three texts, a negative count
    CHECK(refused(16, 3));
    CHECK(refused(23, 0x80));
    CHECK(refused(24 + 12, 1));    // the entry's reserved word
    // bytes behind the last entry
    std::unique_ptr<uint8_t[]> more(new uint8_t[n + 1]);
    memcpy(more.get(), buf, n);
    more[n] = 0;
    Digest x;
    const char *why = digest_read(more.get(), n + 1, &x);
    CHECK(why && !strcmp(why, "is not a scalce digest stream"));
  }
  // T = 2 where one entry follows: the stream ends before its texts do
  uint8_t buf[DIGEST_MAX_BYTES];
  const size_t n = digest_write(buf, sample(0, 1));
  auto e = exact(buf, n);
  e[16] = 2;
  Digest x;
  const char *why = digest_read(e.get(), n, &x);
  CHECK(why && !strcmp(why, "truncated digest stream"));
}

static void messages() {
  char msg[256];
  digest_count_message(msg, sizeof msg, 2, 1);
  CHECK(!strcmp(msg, "digest stream holds 2 texts, the archive 1"));
  DigestText in, got;
  in.bytes = 1000; in.crc = 0x0000BEEFu;
  got.bytes = 999; got.crc = 0xDEADBEEFu;
  digest_mismatch_message(msg, sizeof msg, 1, in, got);
  CHECK(!strcmp(msg, "digest mismatch in text 1: the input had 1000 bytes, crc32 0000beef; written 999 bytes, crc32 deadbeef"));
}

static void arithmetic() {
  const CrcPowers t = crc_powers();
  CHECK(crc_xpow(t, 0) == 0x80000000u && crc_xpow(t, 1) == 0x40000000u && crc_xpow(t, 32) == CRC_POLY);
  CHECK(crc_xpow(t, CRC_ORDER) == 0x80000000u);  // the order of x divides 2^32 - 1
  for (int i = 0; i < 200; i++) {
    const uint32_t a = (uint32_t)rnd(), b = (uint32_t)rnd(), c = (uint32_t)rnd();
    CHECK(crc_mulmod(a, b) == crc_mulmod(b, a));
    CHECK(crc_mulmod(a, 0x80000000u) == a);
    CHECK(crc_mulmod(crc_mulmod(a, b), c) == crc_mulmod(a, crc_mulmod(b, c)));
    const int64_t d = (int64_t)(rnd() >> 24);
    CHECK(crc_mulmod(crc_xpow_bytes(t, d), crc_xpow_bytes(t, -d)) == 0x80000000u);  // a distance and its opposite undo each other
  }
  // against zlib: fixed lengths at the 32-bit edge and beyond, then random pairs
  const uint64_t lens[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 1ull << 40};
  for (uint64_t len : lens)
    for (int i = 0; i < 50; i++) {
      // (an empty B has the CRC 0: zlib versions differ in what they return for other numbers at length 0)
      const uint32_t a = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : (uint32_t)rnd(), b = i == 0 || len == 0 ? 0u : (uint32_t)rnd();
      CHECK(crc32_combine(a, b, len) == (uint32_t)crc32_combine64(a, b, (z_off64_t)len));
      if (len == 0) CHECK(crc32_combine(a, b, len) == a);
    }
  for (int i = 0; i < 2000; i++) {
    const uint32_t a = (uint32_t)rnd(), b = (uint32_t)rnd();
    const uint64_t len = 1 + (rnd() >> (2 + rnd() % 61));
    CHECK(crc32_combine(a, b, len) == (uint32_t)crc32_combine64(a, b, (z_off64_t)len));
  }
  // and against crc32 of real bytes, cut anywhere
  std::vector<uint8_t> text(3000);
  for (auto &v : text) v = (uint8_t)rnd();
  const uint32_t whole = (uint32_t)crc32(0, text.data(), (uInt)text.size());
  for (size_t cut = 0; cut <= text.size(); cut += 37) {
    const uint32_t a = (uint32_t)crc32(0, text.data(), (uInt)cut);
    const uint32_t b = (uint32_t)crc32(0, text.data() + cut, (uInt)(text.size() - cut));
    CHECK(crc32_combine(a, b, text.size() - cut) == whole);
  }
}

int main() {
  round_trip();
  malformed();
  messages();
  arithmetic();
  printf("digeststream_check: ok\n");
  return 0;
}
