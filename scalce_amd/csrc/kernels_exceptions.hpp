// kernels_exceptions.hpp -- the base letters and qualities the archive does not keep (--keep-bases).  The archive stores a base
// as two bits (getval, const.cpp:47-49: a c g t fold to A C G T, every other letter is A) and keeps an upper-case N only through
// quality symbol 0 (qualities.cpp:183; decompress.cpp:350-351 turns every symbol 0 back into N).  With the input's letter b and
// quality character q at a position, the archive gives back
//   symbol  s = 0 if b == 'N', else values[q] - offset            (runs with qualities only)
//   letter  'N' if the run has qualities and s == 0, else "ACGT"[getval(b)]
//   quality offset + s
// and the position is an EXCEPTION when that letter is not b, or when b == 'N' and values[q] != offset (the quality the forced
// symbol lost).  By cases: an N is one when its quality is not the offset; an upper-case A C G T when its quality maps to the
// offset; every other letter always.  Without qualities everything but upper-case A C G T is one.  An entry is a u64:
// letter | values[q] << 8 | position << 16 | record << 28 (PREFIX_<m>.scalcex holds them in archive order).
// Compress side: per piece a count pass over every base and quality byte of the text the ingest read (a u16 per row) and,
// behind an exclusive scan, a write pass that visits the rows with exceptions; the emit stage gathers the entries through the
// permutation and stamps the archive index.  Decompress side: one thread per entry writes it back into a window's text.
#pragma once
#include "kernels_fastq.hpp"
#include "kernels_varlen.hpp"

namespace scalce {

constexpr u32 EXC_LANES = 8;                 // lanes that share a row: 8 x 16 bytes of each line a step, 128 bases
constexpr u32 EXC_ROWS = 256 / EXC_LANES;    // rows per workgroup
constexpr u32 EXC_POS_BITS = 12, EXC_REC_SHIFT = 28;
constexpr u64 EXC_MAX_RECORDS = 1ull << 36;

struct ExcArgs {
  const u8 *text;       // the piece the ingest kernels read (variable-length runs: the padded one)
  u64 nbytes;
  const u64 *line_end;  // its line index
  u32 lpr;              // text lines per record: 4, or 2 (-f)
  u32 unit_recs;        // records per row: 1, or 2 for an interleaved text
  u32 rec0;             // this mate's record inside the unit
  u32 L;
  u32 has_q;            // the run keeps qualities
  int q_affine;         // >= 0: values[c] == c for every c, and this is the offset
  u64 qzero[2];         // else: bit c = values[c] == offset, for the 128 characters,
  u32 qzero_end;        // ... and one more than the highest of them (0: none): a word of qualities at or above it needs no look
  const u8 *qlut;       // (values[c] - offset) & 255, for the entries' quality byte
  u32 qoffset;
  const u16 *padlen;    // variable-length runs: L - length of the piece's rows (the pad is no part of the read); else null
  u64 nrec;             // rows taken from the piece
  u16 *count;           // the piece's rows of the run-wide counts
  const u64 *off;       // write pass: nrec + 1, where each row's entries begin among the piece's
  u64 *dst;             // the store, from the piece's first entry on
  u32 *rows_with;       // per workgroup of the count pass: its rows that hold an exception (summed by a scan: no global atomics)
};

// 16 bytes from any byte address: one 16-byte load where the address allows it, else five aligned words and four v_alignbyte
// (the text begins on a 16-byte boundary; the lines begin at any byte phase)
__device__ __forceinline__ uint4 exc_load16(const u8 *t, u64 at, u64 n) {
  if ((at & 15) == 0 && at + 16 <= n) return *reinterpret_cast<const uint4 *>(t + at);
  const u64 a = at & ~3ull;
  if (a + 20 > n) return vl_load16(t, at, n);
  const u32 sh = (u32)(at & 3);
  const u32 *p = reinterpret_cast<const u32 *>(t + a);
  const u32 w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                    __builtin_amdgcn_alignbyte(w4, w3, sh));
}
// the 0x80 flags of four words -> 16 mask bits (newline_mask16's dot products)
__device__ __forceinline__ u32 exc_mask16(u32 f0, u32 f1, u32 f2, u32 f3) {
  const u32 lo = __builtin_amdgcn_udot4(f1 >> 7, 0x80402010u, __builtin_amdgcn_udot4(f0 >> 7, 0x08040201u, 0u, false), false);
  const u32 hi = __builtin_amdgcn_udot4(f3 >> 7, 0x80402010u, __builtin_amdgcn_udot4(f2 >> 7, 0x08040201u, 0u, false), false);
  return lo | (hi << 8);
}
// 0x80 in every byte of four bases (and their qualities) that is an exception
__device__ __forceinline__ u32 exc_word(const ExcArgs &a, u32 vb, u32 vq) {
  // A | C, G (they differ in bit 2 only) | T
  const u32 acgt = zero_bytes(vb ^ 0x41414141u) | zero_bytes((vb & 0xFBFBFBFBu) ^ 0x43434343u) | zero_bytes(vb ^ 0x54545454u);
  if (!a.has_q) return ~acgt & 0x80808080u;
  const u32 isN = zero_bytes(vb ^ 0x4E4E4E4Eu);
  const u32 x = vq & 0x7F7F7F7Fu;
  u32 qz;  // the quality maps to the offset: symbol 0
  if (a.q_affine >= 0) {
    qz = zero_bytes(x ^ ((u32)a.q_affine * 0x01010101u));
  } else if ((((x | 0x80808080u) - a.qzero_end * 0x01010101u) & 0x80808080u) == 0x80808080u) {
    qz = 0;  // every byte >= qzero_end (no borrow between bytes: each is at least 0x80, qzero_end at most 128): none maps to the offset
  } else {
    qz = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 c = (x >> (8 * k)) & 127u;
      qz |= (u32)((a.qzero[c >> 6] >> (c & 63u)) & 1ull) << (8 * k + 7);
    }
  }
  return ((isN & ~qz) | (~isN & (~acgt | qz))) & 0x80808080u;
}
struct ExcRow { u64 sb, sq; u32 len; };  // where the row's bases and qualities begin in the text; bases that count
__device__ __forceinline__ ExcRow exc_row(const ExcArgs &a, u64 r) {
  const u64 *e = a.line_end + (u64)a.lpr * ((u64)a.unit_recs * r + a.rec0);
  const u64 p0 = e[0], p1 = e[1], p2 = e[a.lpr - 2], p3 = e[a.lpr - 1];
  ExcRow g;
  g.sb = p0 + 1;
  g.sq = p2 + 1;
  // (a record of another length ends the run in the ingest kernel: nothing is made of it here)
  g.len = (p1 - p0 - 1 == (u64)a.L && (a.lpr == 2 || p3 - p2 - 1 == (u64)a.L)) ? a.L : 0u;
  if (a.padlen && g.len) { const u32 pad = a.padlen[r]; g.len = pad < g.len ? g.len - pad : 0u; }
  return g;
}
// bit j: position i + j of the row is an exception (i a multiple of 16, i < len)
__device__ __forceinline__ u32 exc_chunk(const ExcArgs &a, const ExcRow &g, u32 i) {
  const uint4 vb = exc_load16(a.text, g.sb + i, a.nbytes);
  uint4 vq = make_uint4(0, 0, 0, 0);
  if (a.has_q) vq = exc_load16(a.text, g.sq + i, a.nbytes);
  u32 m = exc_mask16(exc_word(a, vb.x, vq.x), exc_word(a, vb.y, vq.y), exc_word(a, vb.z, vq.z), exc_word(a, vb.w, vq.w));
  const u32 rem = g.len - i;
  if (rem < 16) m &= (1u << rem) - 1u;
  return m;
}
// The count pass: EXC_LANES lanes share a row, lane j takes bytes [16 j, 16 j + 16) of every 128 -- a wavefront reads eight
// neighbouring records' sequence and quality lines, every byte once.  LDS: the workgroup's count of rows with an exception.
__global__ __launch_bounds__(256) void exc_count_k(ExcArgs a) {
  __shared__ u32 wg_rows;
  if (threadIdx.x == 0) wg_rows = 0;
  __syncthreads();
  const u32 sub = threadIdx.x & (EXC_LANES - 1);
  const u64 r = (u64)blockIdx.x * EXC_ROWS + threadIdx.x / EXC_LANES;
  u32 cnt = 0;
  if (r < a.nrec) {
    const ExcRow g = exc_row(a, r);
    for (u32 i = sub * 16; i < g.len; i += 16 * EXC_LANES) cnt += (u32)__popc(exc_chunk(a, g, i));
  }
  cnt += __shfl_xor(cnt, 1, 64);
  cnt += __shfl_xor(cnt, 2, 64);
  cnt += __shfl_xor(cnt, 4, 64);
  if (r < a.nrec && sub == 0) {
    a.count[r] = (u16)cnt;
    if (cnt) atomicAdd(&wg_rows, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) a.rows_with[blockIdx.x] = wg_rows;
}
struct ExcNoStore {  // a scan of which only the total is wanted
  __device__ void operator()(u64, u64) const {}
};
struct ExcCount {  // a row's entries
  const u16 *count;
  __device__ u64 operator()(u64 r) const { return count[r]; }
};
// the quality byte of an entry: values[q]
__device__ __forceinline__ u32 exc_quality(const ExcArgs &a, u8 c) {
  if (!a.has_q) return 0u;
  return a.q_affine >= 0 ? (u32)(c & 127u) : ((u32)a.qlut[c & 127u] + a.qoffset) & 255u;
}
// The write pass: the same walk for the rows whose count is not zero (the eight lanes of a row agree on that).  A step's
// entries go behind those of the steps before it, a lane's behind those of the lanes below it: position ascending, every
// place from the scan.
__global__ __launch_bounds__(256) void exc_write_k(ExcArgs a) {
  const u32 sub = threadIdx.x & (EXC_LANES - 1);
  const u64 r = (u64)blockIdx.x * EXC_ROWS + threadIdx.x / EXC_LANES;
  const bool live = r < a.nrec && a.count[r] != 0;
  if (!live) return;
  const ExcRow g = exc_row(a, r);
  const u64 end = a.off[r + 1];
  u64 at = a.off[r];
  for (u32 i0 = 0; i0 < g.len; i0 += 16 * EXC_LANES) {
    const u32 i = i0 + sub * 16;
    u32 m = i < g.len ? exc_chunk(a, g, i) : 0u;
    const u32 c = (u32)__popc(m);
    u32 inc = c;
#pragma unroll
    for (u32 d = 1; d < EXC_LANES; d <<= 1) {
      const u32 t = __shfl_up(inc, d, EXC_LANES);
      if (sub >= d) inc += t;
    }
    const u32 tot = __shfl(inc, EXC_LANES - 1, EXC_LANES);
    u64 o = at + inc - c;
    while (m) {
      const u32 pos = i + (u32)__ffs((int)m) - 1u;
      m &= m - 1;
      if (o < end) a.dst[o] = (u64)a.text[g.sb + pos] | ((u64)exc_quality(a, a.text[g.sq + pos]) << 8) | ((u64)pos << 16);
      o++;
    }
    at += tot;
  }
}

// ---- emit: input order -> archive order ------------------------------------------------------------------------------------
struct ExcCountPermuted {  // the entries of the k-th record of the archive
  const u16 *count;
  const u32 *perm;
  __device__ u64 operator()(u64 k) const { return count[perm[k]]; }
};
// one thread per record of the archive that has entries: they move as they are, the archive index goes into bits 28-63
__global__ __launch_bounds__(256) void exc_gather_k(u64 n, const u32 *perm, const u16 *count, const u64 *in_off, const u64 *in,
                                                    const u64 *out_off, u64 *out) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u64 r = perm[k];
  const u32 c = count[r];
  const u64 *src = in + in_off[r];
  u64 *dst = out + out_off[k];
  for (u32 j = 0; j < c; j++) dst[j] = (src[j] & ((1ull << EXC_REC_SHIFT) - 1)) | (k << EXC_REC_SHIFT);
}

// ---- decompress: apply -----------------------------------------------------------------------------------------------------
struct ExcApplyArgs {
  u8 *text;            // a window's records (fastq_records_k): "@name\n" bases ["\n+\n" qualities] "\n"
  const u64 *rec_off;  // where each record of the text begins, and the text's size
  u32 stride, which;   // record `stride` k + `which` of the text is the window's k-th of this mate (1, 0; interleaved: 2, mate)
  u64 first, nunits;   // the window holds the archive's records (pairs) [first, first + nunits)
  const u64 *entries;
  u64 nent;
  u32 L, has_q;
  u32 *bad;            // set by an entry outside the window or outside its record; such an entry stores nothing
};
// One thread per entry.  The lines lie at fixed distances in front of the record's end (names of any length in front of them).
__global__ __launch_bounds__(256) void exc_apply_k(ExcApplyArgs a) {
  const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= a.nent) return;
  const u64 e = a.entries[x], k = e >> EXC_REC_SHIFT;
  const u32 pos = (u32)(e >> 16) & ((1u << EXC_POS_BITS) - 1u);
  if (k < a.first || k - a.first >= a.nunits || pos >= a.L) { *a.bad = 1u; return; }
  const u64 t = (k - a.first) * a.stride + a.which;
  const u64 start = a.rec_off[t], end = a.rec_off[t + 1];
  const u64 tail = a.has_q ? 2ull * a.L + 5 : (u64)a.L + 2;  // from the header line's newline to the record's end
  if (end < start || end - start < tail + 1) { *a.bad = 1u; return; }
  const u64 last = end - 1 - a.L;  // the record's last line
  if (a.has_q) {
    a.text[last - a.L - 3 + pos] = (u8)e;
    a.text[last + pos] = (u8)(e >> 8);
  } else {
    a.text[last + pos] = (u8)e;
  }
}

// pair_split_k for an interleaved window whose names are made up ("<library>.<index>", -n): mate 2's record is '@', the library
// name, '.', the digits of the pair's archive-wide index and tail2 bytes
__global__ __launch_bounds__(256) void pair_split_lib_k(u64 npairs, const u64 *pair_off, u64 first, u32 lib_len, u64 tail2, u64 *rec_off) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > npairs) return;
  rec_off[2 * k] = pair_off[k];
  if (k == npairs) return;
  const u64 size2 = 2ull + lib_len + fq_digits(first + k) + tail2, e = pair_off[k + 1];
  rec_off[2 * k + 1] = e - pair_off[k] < size2 ? pair_off[k] : e - size2;
}

}  // namespace scalce
