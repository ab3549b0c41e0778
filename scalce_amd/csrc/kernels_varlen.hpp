// kernels_varlen.hpp -- reads of different lengths (params variable_length).  A variable-length run IS the fixed-length run of
// the same records padded to L: in front of the ingest kernels every record of a piece is rewritten with 'N' behind the end of
// its bases and the offset character behind the end of its qualities (an N forces quality symbol 0, qualities.cpp:183, and
// getval packs it as 0), and L - length is kept per row; behind fastq_records_k the pad is cut off again.  Both are copies from
// text to text: one thread per aligned 16-byte granule of the DESTINATION, which finds its record by a search over the records'
// destination offsets (an exclusive scan of their new sizes) inside the few records its workgroup spans.
#pragma once
#include "kernels_ingest.hpp"

namespace scalce {

constexpr u32 VL_CHUNKS = 4;                       // granules per thread
constexpr u32 VL_SPAN = 256u * 16u * VL_CHUNKS;    // destination bytes per workgroup

// 16 bytes from any byte address of a text of n bytes (bytes at or past n read as 0)
__device__ __forceinline__ uint4 vl_load16(const u8 *t, u64 at, u64 n) {
  if ((at & 15) == 0 && at + 16 <= n) return *reinterpret_cast<const uint4 *>(t + at);
  return make_uint4(load_u32_unaligned(t, at, n), load_u32_unaligned(t, at + 4, n), load_u32_unaligned(t, at + 8, n),
                    load_u32_unaligned(t, at + 12, n));
}
// the records a workgroup's span [x0, x1) of the destination meets: the last record that begins at or before x0, and the
// last that begins before x1 (off: n + 1 ascending entries, off[0] = 0)
__device__ __forceinline__ u64 vl_record_of(const u64 *off, u64 lo, u64 hi, u64 x) {  // last r in [lo, hi) with off[r] <= x
  while (hi - lo > 1) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- compress: pad ------------------------------------------------------------------------------------------------------
struct PadArgs {
  const u8 *text;       // the caller's piece
  u64 nbytes;
  const u64 *line_end;  // its line index, four lines per record
  u64 nrec;             // whole records taken from it
  u64 row0;             // run-wide row of the first of them (error messages)
  u32 L;
  u32 qpad;             // the quality pad: the offset character
  u16 *padlen;          // per record: L - length
  u64 *dst_off;         // nrec + 1: where each record begins in the padded text, and the text's size
  u8 *dst;
  DevErr *err;
};
// one thread per record: its length against L and against its quality line's, L - length into the row array
__global__ __launch_bounds__(256) void pad_plan_k(PadArgs a) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrec) return;
  const u64 *e = a.line_end + 4 * r;
  const u64 ls = e[1] - e[0] - 1, lq = e[3] - e[2] - 1;
  u32 pad = 0;  // (a record that fails is copied as it is: the run ends with the error)
  if (ls != lq) dev_fail(a.err, E_SEQQUAL, a.row0 + r, (u32)(ls < 0xFFFFFFFFull ? ls : 0xFFFFFFFFull));
  else if (ls > (u64)a.L) dev_fail(a.err, E_READLEN, a.row0 + r, (u32)(ls < 0xFFFFFFFFull ? ls : 0xFFFFFFFFull));
  else pad = a.L - (u32)ls;
  a.padlen[r] = (u16)pad;
}
struct PaddedSize {  // a record's bytes once padded
  const u64 *line_end;
  const u16 *padlen;
  __device__ u64 operator()(u64 r) const {
    return line_end[4 * r + 3] + 1 - (r ? line_end[4 * r - 1] + 1 : 0) + 2ull * padlen[r];
  }
};
// A padded record is five runs: [name line, bases) from the text, `pad` x 'N', [newline, '+' line, qualities) from the text,
// `pad` x the quality pad, the newline.  A granule inside one run is one 16-byte store of bytes fetched from any byte phase
// of the source (or of the pad character); a granule that meets a seam is put together byte by byte.
__global__ __launch_bounds__(256) void pad_copy_k(PadArgs a) {
  __shared__ u64 r_span[2];
  const u64 total = a.dst_off[a.nrec];
  const u64 span0 = (u64)blockIdx.x * VL_SPAN;
  if (span0 >= total) return;
  const u64 span1 = span0 + VL_SPAN < total ? span0 + VL_SPAN : total;
  if (threadIdx.x < 2) r_span[threadIdx.x] = vl_record_of(a.dst_off, 0, a.nrec, threadIdx.x ? span1 - 1 : span0);
  __syncthreads();
  const u64 r_lo = r_span[0], r_hi = r_span[1] + 1;
#pragma unroll 1
  for (u32 c = 0; c < VL_CHUNKS; c++) {
    const u64 x0 = span0 + ((u64)c * 256u + threadIdx.x) * 16u;
    if (x0 >= total) break;
    const u64 x1 = x0 + 16 < total ? x0 + 16 : total;
    u64 r = vl_record_of(a.dst_off, r_lo, r_hi, x0);
    // the record's runs, in destination bytes from its start
    u64 d0, ns, p1, A, B, pad, size;
    auto view = [&](u64 rr) {
      const u64 *e = a.line_end + 4 * rr;
      d0 = a.dst_off[rr];
      ns = rr ? e[-1] + 1 : 0;
      p1 = e[1];
      pad = a.padlen[rr];
      A = p1 - ns;       // name line and bases
      B = e[3] - p1;     // the newline behind the bases, the '+' line, the qualities
      size = A + B + 2 * pad + 1;
    };
    view(r);
    const u64 j0 = x0 - d0;
    if (x1 - x0 == 16 && j0 + 16 <= size) {
      bool whole = true;
      uint4 v;
      if (j0 + 16 <= A) v = vl_load16(a.text, ns + j0, a.nbytes);
      else if (j0 >= A && j0 + 16 <= A + pad) v = make_uint4(0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu);
      else if (j0 >= A + pad && j0 + 16 <= A + pad + B) v = vl_load16(a.text, p1 + (j0 - A - pad), a.nbytes);
      else if (j0 >= A + pad + B && j0 + 16 <= A + 2 * pad + B) { const u32 q = a.qpad * 0x01010101u; v = make_uint4(q, q, q, q); }
      else whole = false;
      if (whole) { *reinterpret_cast<uint4 *>(a.dst + x0) = v; continue; }
    }
    for (u64 x = x0; x < x1; x++) {
      while (x - d0 >= size) view(++r);  // (x < total: there is such a record)
      const u64 j = x - d0;
      u8 ch;
      if (j < A) ch = a.text[ns + j];
      else if (j < A + pad) ch = 'N';
      else if (j < A + pad + B) ch = a.text[p1 + (j - A - pad)];
      else if (j < A + 2 * pad + B) ch = (u8)a.qpad;
      else ch = '\n';
      a.dst[x] = ch;
    }
  }
}

// L - length of the rows in output order (SCALCE_OUT_LENGTHS)
__global__ __launch_bounds__(256) void gather_padlen_k(u64 n, const u32 *perm, const u16 *in, u16 *out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[perm[i]];
}

// ---- decompress: strip --------------------------------------------------------------------------------------------------
struct StripArgs {
  const u8 *text;       // a window's padded records (fastq_records_k): "@name\n" bases "\n+\n" qualities "\n"
  const u64 *rec_off;   // nrec + 1: where each begins, and the text's size
  const u8 *entries;    // the window's entries of the length stream, `width` bytes each, little-endian: L - length
  u32 width, L;
  u64 nrec;
  u64 *dst_off;         // nrec + 1: the same for the stripped text
  u8 *dst;
};
__device__ __forceinline__ u32 strip_pad(const StripArgs &a, u64 r) {
  const u32 p = a.width == 2 ? (u32)a.entries[2 * r] | ((u32)a.entries[2 * r + 1] << 8) : (u32)a.entries[r];
  return p < a.L ? p : a.L;  // (an entry beyond L is refused on the host; here it must not reach in front of the record)
}
struct StrippedSize {
  StripArgs a;
  __device__ u64 operator()(u64 r) const { return a.rec_off[r + 1] - a.rec_off[r] - 2ull * strip_pad(a, r); }
};
// A stripped record is three runs of the padded one: [name line, the first `len` bases), then the newline, the '+' line and
// the first `len` qualities, then the newline.  The lines lie at fixed distances in front of the record's end.
__global__ __launch_bounds__(256) void strip_copy_k(StripArgs a) {
  __shared__ u64 r_span[2];
  const u64 total = a.dst_off[a.nrec], nsrc = a.rec_off[a.nrec];
  const u64 span0 = (u64)blockIdx.x * VL_SPAN;
  if (span0 >= total) return;
  const u64 span1 = span0 + VL_SPAN < total ? span0 + VL_SPAN : total;
  if (threadIdx.x < 2) r_span[threadIdx.x] = vl_record_of(a.dst_off, 0, a.nrec, threadIdx.x ? span1 - 1 : span0);
  __syncthreads();
  const u64 r_lo = r_span[0], r_hi = r_span[1] + 1;
  const u64 L = a.L;
#pragma unroll 1
  for (u32 c = 0; c < VL_CHUNKS; c++) {
    const u64 x0 = span0 + ((u64)c * 256u + threadIdx.x) * 16u;
    if (x0 >= total) break;
    const u64 x1 = x0 + 16 < total ? x0 + 16 : total;
    u64 r = vl_record_of(a.dst_off, r_lo, r_hi, x0);
    u64 d0, s0, mid, A, B, size;
    auto view = [&](u64 rr) {
      const u64 e = a.rec_off[rr + 1], len = L - strip_pad(a, rr);
      d0 = a.dst_off[rr];
      s0 = a.rec_off[rr];
      mid = e - L - 4;                    // the newline behind the bases
      A = (e - 2 * L - 4 - s0) + len;     // name line and the bases kept
      B = 3 + len;                        // "\n+\n" and the qualities kept
      size = A + B + 1;
    };
    view(r);
    const u64 j0 = x0 - d0;
    if (x1 - x0 == 16 && j0 + 16 <= size) {
      if (j0 + 16 <= A) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, s0 + j0, nsrc); continue; }
      if (j0 >= A && j0 + 16 <= A + B) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, mid + (j0 - A), nsrc); continue; }
    }
    for (u64 x = x0; x < x1; x++) {
      while (x - d0 >= size) view(++r);
      const u64 j = x - d0;
      a.dst[x] = j < A ? a.text[s0 + j] : j < A + B ? a.text[mid + (j - A)] : (u8)'\n';
    }
  }
}

}  // namespace scalce
