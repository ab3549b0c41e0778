// digeststream.hpp -- the digest stream of an archive made with --lossless --digest (PREFIX_1.scalced), host side only: no
// device call, no HIP header.  Layout (sidestream.hpp): the 8 magic bytes, int32 16 (entry width), int32 kind, int64 T (texts: 1 or 2), then T
// entries of {u64 bytes, u32 crc32, u32 0}, little-endian.  kind: 0 one text, 1 paired files (-r), 2 interleaved (-i); + 4 for
// two-line records (-f).  The CRC-32 is zlib's (polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF) of the
// text of one mate stream as the run read it.  The writer and the reader (cli.cpp) share it, and with the device kernel
// (kernels_crc.hpp) the arithmetic that joins the CRCs of pieces: a multiplication by x^(8 len) modulo the polynomial.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "sidestream.hpp"

#ifdef __HIPCC__
#define SCALCE_CRC_HD __host__ __device__
#else
#define SCALCE_CRC_HD
#endif

namespace scalce_host {

// ---- CRC-32 arithmetic.  A 32-bit word holds a polynomial over GF(2) reflected, as the CRC register does: bit 31 is x^0.
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint64_t CRC_ORDER = 0xFFFFFFFFull;  // x^(2^32 - 1) = 1: the modulus is irreducible of degree 32

// a(x) b(x) mod P
SCALCE_CRC_HD inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
  }
  return p;
}
// x^(2^k) mod P for k = 0 .. 31
struct CrcPowers { uint32_t x2k[32]; };
inline CrcPowers crc_powers() {
  CrcPowers t;
  t.x2k[0] = 0x40000000u;  // x^1
  for (int k = 1; k < 32; k++) t.x2k[k] = crc_mulmod(t.x2k[k - 1], t.x2k[k - 1]);
  return t;
}
// x^e mod P, e < 2^32
SCALCE_CRC_HD inline uint32_t crc_xpow(const CrcPowers &t, uint64_t e) {
  uint32_t p = 0x80000000u;  // x^0
  for (int k = 0; k < 32 && e; k++, e >>= 1)
    if (e & 1) p = crc_mulmod(t.x2k[k], p);
  return p;
}
// x^(8 bytes) mod P for a distance of any sign: exponents count modulo the order of x
SCALCE_CRC_HD inline uint32_t crc_xpow_bytes(const CrcPowers &t, int64_t bytes) {
  const uint64_t mag = (uint64_t)(bytes < 0 ? -bytes : bytes) % CRC_ORDER;
  uint64_t e = mag * 8 % CRC_ORDER;
  if (bytes < 0 && e) e = CRC_ORDER - e;
  return crc_xpow(t, e);
}
// crc32(A || B) from crc32(A), crc32(B) and B's length: zlib's crc32_combine64
inline uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  static const CrcPowers t = crc_powers();
  return crc_mulmod(crc_xpow(t, (len_b % CRC_ORDER) * 8 % CRC_ORDER), crc_a) ^ crc_b;
}

// ---- the stream
constexpr size_t DIGEST_HEADER_BYTES = side_header_bytes(1);
constexpr int DIGEST_ENTRY_WIDTH = 16;
constexpr int DIGEST_KIND_SINGLE = 0, DIGEST_KIND_PAIRED = 1, DIGEST_KIND_INTERLEAVED = 2, DIGEST_KIND_FASTA = 4;

struct DigestText { uint64_t bytes = 0; uint32_t crc = 0; };
struct Digest {
  int kind = 0;
  int texts = 0;
  DigestText text[2];
};
constexpr size_t DIGEST_MAX_BYTES = DIGEST_HEADER_BYTES + 2 * DIGEST_ENTRY_WIDTH;

// the whole stream into out (DIGEST_MAX_BYTES of room); returns its size
inline size_t digest_write(uint8_t *out, const Digest &d) {
  side_header_write(out, 1, SideHeader{DIGEST_ENTRY_WIDTH, (int32_t)d.kind, {d.texts}});
  for (int i = 0; i < d.texts; i++) {
    uint8_t *e = out + DIGEST_HEADER_BYTES + (size_t)i * DIGEST_ENTRY_WIDTH;
    const uint32_t w[2] = {d.text[i].crc, 0};
    memcpy(e, &d.text[i].bytes, 8);
    memcpy(e + 8, w, 8);
  }
  return DIGEST_HEADER_BYTES + (size_t)d.texts * DIGEST_ENTRY_WIDTH;
}
// nullptr: a stream this build reads (*d filled in); else what is wrong with it.  `have` = every byte of the stream.
inline const char *digest_read(const uint8_t *h, size_t have, Digest *d) {
  SideHeader f;
  const SideHeaderState st = side_header_read(h, have, 1, &f);
  if (st == SIDE_SHORT) return "truncated digest stream";
  const int64_t t = f.count[0];
  if (st == SIDE_NOT_OURS || f.width != DIGEST_ENTRY_WIDTH || f.param < 0 || f.param > 7 || (f.param & 3) == 3 || (t != 1 && t != 2))
    return "is not a scalce digest stream";
  if (have < DIGEST_HEADER_BYTES + (size_t)t * DIGEST_ENTRY_WIDTH) return "truncated digest stream";
  if (have > DIGEST_HEADER_BYTES + (size_t)t * DIGEST_ENTRY_WIDTH) return "is not a scalce digest stream";
  d->kind = f.param;
  d->texts = (int)t;
  for (int i = 0; i < d->texts; i++) {
    const uint8_t *e = h + DIGEST_HEADER_BYTES + (size_t)i * DIGEST_ENTRY_WIDTH;
    uint32_t w[2];
    memcpy(&d->text[i].bytes, e, 8);
    memcpy(w, e + 8, 8);
    if (w[1] != 0) return "is not a scalce digest stream";
    d->text[i].crc = w[0];
  }
  return nullptr;
}
// texts the kind implies: two for paired files, one otherwise
inline int digest_kind_texts(int kind) { return (kind & 3) == DIGEST_KIND_PAIRED ? 2 : 1; }
inline int digest_count_message(char *out, size_t cap, uint64_t texts, uint64_t archive) {
  return snprintf(out, cap, "digest stream holds %llu texts, the archive %llu", (unsigned long long)texts, (unsigned long long)archive);
}
inline int digest_mismatch_message(char *out, size_t cap, int text, const DigestText &in, const DigestText &got) {
  return snprintf(out, cap, "digest mismatch in text %d: the input had %llu bytes, crc32 %08x; written %llu bytes, crc32 %08x", text,
                  (unsigned long long)in.bytes, in.crc, (unsigned long long)got.bytes, got.crc);
}

}  // namespace scalce_host
