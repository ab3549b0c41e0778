// kernels_crc.hpp -- zlib's CRC-32 of a text that lies on the device (--digest, and the check on -d).  One memory-bound read.
//
// The register of a CRC is a polynomial modulo P, and everything here is linear over GF(2): with raw(M) the register after M
// from a zero start and without the final xor, raw(A || B) = raw(A) x^(8 |B|) + raw(B), and zeros in FRONT of a message change
// nothing.  gfx950 has no carry-less multiply, so a product with a FIXED power of x is a table probe per nibble of the word.
//
// Shape.  The bytes are laid on a grid of 16-byte granules aligned in MEMORY (the range's head and tail granules are read byte
// by byte, inside the range only; what lies outside counts as zero).  A workgroup of 1024 lanes takes a SPAN of whole TILES of
// 16 KiB; in each tile lane l loads granule l -- a wave reads 1 KiB in one coalesced 16-byte load per lane -- and folds it
// into its own register: s = s x^(8 TILE) + w0 x^(8 16) + w1 x^(8 12) + w2 x^(8 8) + w3 x^(8 4), five words, eight nibble
// probes each.  The 40 tables of 16 entries stand in LDS once PER BANK (entry e of table j for lane l at dword (j 16 + e) 32 +
// l % 32), so a ds_read_b32 of a wave, which the LDS serves in two groups of 32 lanes over 32 banks, never meets a conflict
// whatever the data is: 80 KiB.  Behind the span lane l multiplies its register by x^(8 16 (1023 - l)) (a general product, once
// per launch), the workgroup xors the lanes together and stores one word.  A second, small launch multiplies each workgroup's
// word by the power of x that its span's end lies in front of the range's end -- negative for the last one, whose span is
// padded with zeros: exponents count modulo 2^32 - 1 --, xors them, and adds the initial value's share and the final xor.
#pragma once
#include "digeststream.hpp"
#include "prims.hpp"

namespace scalce {

constexpr u32 CRC_GRANULE = 16;                      // bytes per lane per step
constexpr u32 CRC_THREADS = 1024;
constexpr u32 CRC_TILE = CRC_GRANULE * CRC_THREADS;  // bytes per workgroup per step
constexpr u32 CRC_MAX_WG = 512;
constexpr u32 CRC_TABLES = 40;
constexpr u32 CRC_LDS_BYTES = CRC_TABLES * 16 * 32 * 4;
constexpr u64 CRC_MAX_BYTES = 1ull << 40;            // (a span stays below 2^32 bytes)

struct CrcPlan { u32 tile_count_per_span; u32 span; u32 wgs; };
// tiles of the grid that holds `head` bytes in front of the range (its start's offset in its granule) and the range
inline bool crc_plan(u64 head, u64 nbytes, CrcPlan *p) {
  if (nbytes > CRC_MAX_BYTES || head >= CRC_GRANULE) return false;
  const u64 tiles = (head + nbytes + CRC_TILE - 1) / CRC_TILE;
  const u64 per = tiles ? (tiles + CRC_MAX_WG - 1) / CRC_MAX_WG : 1;
  p->tile_count_per_span = (u32)per;
  p->span = (u32)(per * CRC_TILE);
  p->wgs = (u32)((tiles + per - 1) / per);
  return true;
}

struct CrcArgs {
  const u8 *base;    // the range's start rounded down to a granule
  u64 lo, hi;        // the range in bytes behind base: [lo, hi), lo < 16
  u32 tiles_per_span;
  u32 *partial;      // one word per workgroup
  u32 *out;
  u32 nwg;
  scalce_host::CrcPowers pw;
};

__device__ __forceinline__ u32 crc_probe(const u32 *tab, u32 table, u32 word, u32 nib) {
  return tab[((table * 8 + nib) * 16 + ((word >> (4 * nib)) & 15u)) * 32];
}
// (tab: the lane's bank column of the tables)
__device__ __forceinline__ u32 crc_fold(const u32 *tab, u32 s, u32x4 w) {
  u32 r = 0;
#pragma unroll
  for (u32 nib = 0; nib < 8; nib++) {
    r ^= crc_probe(tab, 0, w.x, nib) ^ crc_probe(tab, 1, w.y, nib);
    r ^= crc_probe(tab, 2, w.z, nib) ^ crc_probe(tab, 3, w.w, nib);
    r ^= crc_probe(tab, 4, s, nib);
  }
  return r;
}
// a granule that the range's ends cut: byte loads inside [lo, hi) only
__device__ inline u32x4 crc_edge_granule(const u8 *base, u64 at, u64 lo, u64 hi) {
  u32 w[4] = {0, 0, 0, 0};
  for (u32 i = 0; i < CRC_GRANULE; i++) {
    const u64 p = at + i;
    if (p >= lo && p < hi) w[i >> 2] |= (u32)base[p] << (8 * (i & 3));
  }
  u32x4 v;
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  return v;
}

__global__ __launch_bounds__(CRC_THREADS) void crc32_span_k(CrcArgs a) {
  extern __shared__ __attribute__((aligned(16))) u32 crc_tab[];
  __shared__ u32 wave_x[CRC_THREADS / 64];
  __shared__ u32 tab_value[CRC_TABLES * 16];
  const u32 tid = threadIdx.x;
  // the tables: entry e of nibble n of word k is (e << 4 n) x^(8 d_k), d = 16, 12, 8, 4 for the granule's words, TILE for the register
  // (values first, then every lane writes its share of the bank copies: consecutive lanes, consecutive dwords)
  if (tid < CRC_TABLES * 16) {
    const u32 k = tid >> 7, nib = (tid >> 4) & 7, e = tid & 15;
    const u32 dist = k < 4 ? 16 - 4 * k : CRC_TILE;
    tab_value[tid] = scalce_host::crc_mulmod(e << (4 * nib), scalce_host::crc_xpow(a.pw, 8ull * dist));
  }
  __syncthreads();
  for (u32 i = tid; i < CRC_TABLES * 16 * 32; i += CRC_THREADS) crc_tab[i] = tab_value[i >> 5];
  __syncthreads();
  const u32 *tab = crc_tab + (tid & 31);
  const u64 span0 = (u64)blockIdx.x * a.tiles_per_span * CRC_TILE;
  const u8 *p = a.base + span0 + (u64)tid * CRC_GRANULE;
  u32 s = 0;
#pragma unroll 1
  for (u32 t = 0; t < a.tiles_per_span;) {
    const u64 t0 = span0 + (u64)t * CRC_TILE;
    if (t + 4 <= a.tiles_per_span && t0 >= a.lo && t0 + 4ull * CRC_TILE <= a.hi) {
      // four whole tiles inside the range: four loads in flight per lane
      const u32x4 w0 = *reinterpret_cast<const u32x4 *>(p + (u64)t * CRC_TILE);
      const u32x4 w1 = *reinterpret_cast<const u32x4 *>(p + (u64)(t + 1) * CRC_TILE);
      const u32x4 w2 = *reinterpret_cast<const u32x4 *>(p + (u64)(t + 2) * CRC_TILE);
      const u32x4 w3 = *reinterpret_cast<const u32x4 *>(p + (u64)(t + 3) * CRC_TILE);
      s = crc_fold(tab, s, w0);
      s = crc_fold(tab, s, w1);
      s = crc_fold(tab, s, w2);
      s = crc_fold(tab, s, w3);
      t += 4;
    } else {
      // a tile that one of the range's ends cuts, one of the span's last, or one behind the range (zeros: the register moves on alone)
      const u64 at = t0 + (u64)tid * CRC_GRANULE;
      u32x4 w;
      w.x = w.y = w.z = w.w = 0;
      if (at >= a.lo && at + CRC_GRANULE <= a.hi)
        w = *reinterpret_cast<const u32x4 *>(a.base + at);
      else if (at + CRC_GRANULE > a.lo && at < a.hi)
        w = crc_edge_granule(a.base, at, a.lo, a.hi);
      s = crc_fold(tab, s, w);
      t += 1;
    }
  }
  // the lanes' registers end 16 bytes apart: lane l's lies 16 (1023 - l) bytes in front of the span's end
  s = scalce_host::crc_mulmod(s, scalce_host::crc_xpow(a.pw, 8ull * CRC_GRANULE * (CRC_THREADS - 1 - tid)));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s ^= __shfl_xor(s, d, 64);
  if ((tid & 63) == 0) wave_x[tid >> 6] = s;
  __syncthreads();
  if (tid < 64) {
    u32 v = tid < CRC_THREADS / 64 ? wave_x[tid] : 0;
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    if (tid == 0) a.partial[blockIdx.x] = v;
  }
}

// one workgroup: the spans' words to the range's end, the initial value's share, the final xor
__global__ __launch_bounds__(256) void crc32_join_k(CrcArgs a) {
  __shared__ u32 wave_x[4];
  const u32 tid = threadIdx.x;
  const u64 span = (u64)a.tiles_per_span * CRC_TILE;
  u32 s = 0;
  for (u32 g = tid; g < a.nwg; g += 256) {
    const long long dist = (long long)a.hi - (long long)((u64)(g + 1) * span);
    s ^= scalce_host::crc_mulmod(a.partial[g], scalce_host::crc_xpow_bytes(a.pw, dist));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s ^= __shfl_xor(s, d, 64);
  if ((tid & 63) == 0) wave_x[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    const u32 raw = wave_x[0] ^ wave_x[1] ^ wave_x[2] ^ wave_x[3];
    const u32 init = scalce_host::crc_mulmod(0xFFFFFFFFu, scalce_host::crc_xpow_bytes(a.pw, (long long)(a.hi - a.lo)));
    a.out[0] = raw ^ init ^ 0xFFFFFFFFu;
  }
}

}  // namespace scalce
