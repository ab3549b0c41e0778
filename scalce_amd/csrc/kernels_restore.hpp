// kernels_restore.hpp -- part of scalce_hip.hip (included there behind the host_*.inc files): the device side of the order
// restore (archives made with --keep-order).  The records of a window belong at places spread over the whole output, so the
// output is cut into STRIPES of R consecutive input indices and the records travel in two passes: a window's records are
// grouped by stripe (scalce_order_group + scalce_records_permute) and spilled; a stripe's records, gathered from every window's
// spill, are put in their places (scalce_order_place + scalce_records_permute).  Neither looks inside a record.
//
// The copy is driven by the DESTINATION like strip_copy_k: a workgroup owns VL_SPAN bytes of the output in 16-byte granules,
// finds the records its span meets by one binary search over the output offsets, and a granule that lies inside one record
// is one 16-byte load from any byte phase of the source and one aligned 16-byte store -- a wavefront's stores are one
// contiguous run of 1 KiB, its loads runs of a record's length.  Granules that meet a record boundary go byte by byte.
#pragma once
#include "kernels_varlen.hpp"

namespace scalce {

struct PermuteArgs {
  const u8 *text;      // the source text, moved back to a 16-byte boundary: record bytes begin `shift` later
  u64 shift, nsrc;     // nsrc: bytes of the source from `text` on (shift included)
  const u64 *src_off;  // nrec + 1: where each source record begins
  const u32 *source;   // nrec: output record r is source record source[r]
  u64 nrec;
  u64 *dst_off;        // nrec + 1
  u8 *dst;
  u64 dst_cap;         // bytes dst holds: nothing is stored at or past it
};
struct PermutedSize {  // (an entry that names no record gives an empty one: the caller's d_bad says why)
  const u64 *src_off;
  const u32 *source;
  u64 nrec;
  __device__ u64 operator()(u64 r) const {
    const u64 q = source[r];
    return q < nrec ? src_off[q + 1] - src_off[q] : 0;
  }
};
__global__ __launch_bounds__(256) void permute_copy_k(PermuteArgs a) {
  __shared__ u64 r_span[2];
  u64 total = a.dst_off[a.nrec];
  if (total > a.dst_cap) total = a.dst_cap;
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
    u64 d0, s0, size;
    auto view = [&](u64 rr) {
      const u64 q = a.source[rr];
      d0 = a.dst_off[rr];
      size = a.dst_off[rr + 1] - d0;  // (0 for an entry that names no record: never read from)
      s0 = (q < a.nrec ? a.src_off[q] : 0) + a.shift;
    };
    view(r);
    const u64 j0 = x0 - d0;
    if (x1 - x0 == 16 && j0 + 16 <= size) {
      *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, s0 + j0, a.nsrc);
      continue;
    }
    for (u64 x = x0; x < x1; x++) {
      while (x - d0 >= size) view(++r);  // (x < total <= dst_off[nrec]: there is such a record)
      a.dst[x] = a.text[s0 + (x - d0)];
    }
  }
}

// ---- grouping a window's records by stripe --------------------------------------------------------------------------------
struct StripeDigit {  // 8 bits of the stripe of record v of the window
  const u32 *index;
  u32 R, last, shift;
  __device__ u32 stripe(u32 v) const {
    const u32 s = index[v] / R;
    return s < last ? s : last;  // (an index beyond the records is reported through d_bad; here it must stay a stripe)
  }
  __device__ u32 operator()(u32 v) const { return (stripe(v) >> shift) & 0xFFu; }
};
__global__ __launch_bounds__(256) void order_range_k(const u32 *index, u64 n, u64 total, u32 *bad) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (u64)index[i] >= total) *bad = 1;
}
// start[s] = how many of the grouped records lie in stripes below s (S + 1 entries): position k opens every stripe between
// its left neighbour's and its own, position n those behind the last -- each entry has one writer
__global__ __launch_bounds__(256) void stripe_starts_k(StripeDigit d, const u32 *source, u64 n, u32 S, u32 *start) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n) return;
  const u32 lo = k ? d.stripe(source[k - 1]) + 1 : 0;
  const u32 hi = k < n ? d.stripe(source[k]) : S;
  for (u32 s = lo; s <= hi && s <= S; s++) start[s] = (u32)k;
}
__global__ __launch_bounds__(256) void stripe_counts_k(const u32 *start, u32 S, u32 *counts) {
  const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) counts[s] = start[s + 1] - start[s];
}

// ---- a stripe's records into their places ---------------------------------------------------------------------------------
// scatter, then verify: of two records that claim one place one store wins, and the other record sees it
__global__ __launch_bounds__(256) void place_scatter_k(const u32 *index, u64 m, u64 base, u64 expect, u32 *source, u32 *bad) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && m != expect) *bad = 1;  // (a place stays empty, or is claimed twice)
  if (i >= m) return;
  const u64 x = index[i];
  if (x < base || x - base >= expect) { *bad = 1; return; }
  source[x - base] = (u32)i;
}
__global__ __launch_bounds__(256) void place_verify_k(const u32 *index, u64 m, u64 base, u64 expect, const u32 *source, u32 *bad) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const u64 x = index[i];
  if (x >= base && x - base < expect && source[x - base] != (u32)i) *bad = 1;
}

}  // namespace scalce

// ---- the C ABI ------------------------------------------------------------------------------------------------------------
extern "C" uint64_t scalce_records_permute_ws_bytes(uint64_t nrecords) { return sizeof(u64) * (scan_ws_elems(nrecords) + 64); }
extern "C" int scalce_records_permute(scalce_ctx *c, const uint8_t *d_text, const uint64_t *d_record_offsets, uint64_t nrecords,
                                      uint64_t text_bytes, const uint32_t *d_source, uint8_t *d_out, uint64_t out_cap,
                                      uint64_t *d_out_offsets, void *d_ws, void *stream) {
  if (!c || !d_out_offsets || !d_ws || nrecords > 0xFFFFFFFFull) return SCALCE_ERR_ARG;
  if (nrecords && (!d_text || !d_record_offsets || !d_source || !d_out)) return SCALCE_ERR_ARG;
  if ((uintptr_t)d_out & 15) { set_err(c, "permute: the output text must be 16-byte aligned"); return SCALCE_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  PermuteArgs a;
  a.shift = (u64)((uintptr_t)d_text & 15);
  a.text = d_text - a.shift;
  a.nsrc = text_bytes + a.shift;
  a.src_off = reinterpret_cast<const u64 *>(d_record_offsets); a.source = d_source; a.nrec = nrecords;
  a.dst_off = reinterpret_cast<u64 *>(d_out_offsets); a.dst = d_out; a.dst_cap = out_cap;
  exclusive_scan<u64>(PermutedSize{a.src_off, a.source, nrecords}, nrecords, StoreTo<u64>{a.dst_off}, static_cast<u64 *>(d_ws),
                      a.dst_off + nrecords, s);
  // (the grid covers what the output can hold at most, known without a read-back; workgroups behind the text's end return)
  const u64 bound = std::min<u64>(out_cap, text_bytes);
  if (nrecords && bound) LAUNCH(permute_copy_k, cdiv(bound, VL_SPAN), 256, 0, s, a);
  return launch_failed(c);
}

// scratch of scalce_order_group: the other half of the radix passes, their histogram and scan tiles, the stripes' starts
static u64 order_group_ws_words(u64 n, u64 S) {
  return (n + 64) + radix_hist_elems(n) + 2 * (scan_ws_elems(radix_hist_elems(n)) + 64) + (S + 64);
}
extern "C" uint64_t scalce_order_group_ws_bytes(uint64_t nrecords, uint64_t nstripes) { return sizeof(u32) * order_group_ws_words(nrecords, nstripes); }
extern "C" int scalce_order_group(scalce_ctx *c, const uint32_t *d_index, uint64_t nrecords, uint64_t stripe_records, uint64_t total_records,
                                  uint64_t nstripes, uint32_t *d_source, uint32_t *d_stripe_counts, uint32_t *d_bad, void *d_ws, void *stream) {
  if (!c || !d_bad || !d_ws || !stripe_records || stripe_records > 0xFFFFFFFFull || total_records > 0xFFFFFFFFull ||
      nrecords > 0x7FFFFFFFull || nstripes > 65536 || (nstripes && !d_stripe_counts))
    return SCALCE_ERR_ARG;
  if (nrecords && (!d_index || !d_source || !nstripes)) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(u32), s));
  const u32 n = (u32)nrecords, S = (u32)nstripes;
  u32 *tmp = static_cast<u32 *>(d_ws), *hist = tmp + (n + 64), *tiles = hist + radix_hist_elems(n);
  u32 *start = tiles + 2 * (scan_ws_elems(radix_hist_elems(n)) + 64);
  StripeDigit d{d_index, (u32)stripe_records, S ? S - 1 : 0, 0};
  if (n) {
    LAUNCH(order_range_k, cdiv(n, 256), 256, 0, s, d_index, nrecords, total_records, d_bad);
    if (S > 256) {  // two stable passes of 8 bits: the low byte of the stripe, then the high one
      radix_pass((const u32 *)nullptr, tmp, n, d, hist, tiles, s);
      StripeDigit hi = d;
      hi.shift = 8;
      radix_pass(tmp, d_source, n, hi, hist, tiles, s);
    } else {
      radix_pass((const u32 *)nullptr, d_source, n, d, hist, tiles, s);
    }
  }
  if (S) {
    LAUNCH(stripe_starts_k, cdiv((u64)n + 1, 256), 256, 0, s, d, d_source, nrecords, S, start);
    LAUNCH(stripe_counts_k, cdiv(S, 256), 256, 0, s, start, S, d_stripe_counts);
  }
  return launch_failed(c);
}

extern "C" int scalce_order_place(scalce_ctx *c, const uint32_t *d_index, uint64_t m, uint64_t base, uint64_t expect, uint32_t *d_source,
                                  uint32_t *d_bad, void *stream) {
  if (!c || !d_bad || m > 0xFFFFFFFFull || expect > 0xFFFFFFFFull || (m && !d_index) || (expect && !d_source)) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(u32), s));
  if (expect) HIP_TRY(c, hipMemsetAsync(d_source, 0xFF, sizeof(u32) * expect, s));  // an empty place names no record
  LAUNCH(place_scatter_k, cdiv(std::max<u64>(m, 1), 256), 256, 0, s, d_index, m, base, expect, d_source, d_bad);
  if (m) LAUNCH(place_verify_k, cdiv(m, 256), 256, 0, s, d_index, m, base, expect, d_source, d_bad);
  return launch_failed(c);
}

// out[k] = in[source[k]]: the grouped records' entries of the order stream (what the spill keeps per record)
namespace scalce {
__global__ __launch_bounds__(256) void gather_u32_k(u64 n, const u32 *source, const u32 *in, u32 *out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[source[i]];
}
}  // namespace scalce
extern "C" int scalce_order_gather(scalce_ctx *c, const uint32_t *d_in, const uint32_t *d_source, uint64_t n, uint32_t *d_out, void *stream) {
  if (!c || (n && (!d_in || !d_source || !d_out))) return SCALCE_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  if (n) LAUNCH(gather_u32_k, cdiv(n, 256), 256, 0, (hipStream_t)stream, n, d_source, d_in, d_out);
  return launch_failed(c);
}
