// kernels_comments.hpp -- what follows the name on a record's header line (--keep-comments).  The name slicer stops at the first
// space (output_name, names.cpp:55-57); the bytes from that space to the newline, the record's ENTRY, go into a stream of their
// own (PREFIX_<m>.scalcec), one newline-terminated entry per record in archive order.  Compress side: per piece a plan pass
// (entry length per row, u16) and an extract pass (the entries, each with its newline, appended to a per-mate byte store in
// input order); the emit stage gathers the store through the permutation with permute_copy_k (kernels_restore.hpp).
// Decompress side: an insert pass puts a window's entries back between each name and its newline.
#pragma once
#include "kernels_varlen.hpp"

namespace scalce {

constexpr u32 COM_MAX = 65535;            // the longest entry kept (its length is a u16 row)
constexpr u32 COM_CHUNKS = 16;            // destination bytes per thread of comment_copy_k
constexpr u32 COM_SPAN = 256u * COM_CHUNKS;

// where the first byte of text[i, end) that equals `four`'s (one byte, four times over) lies, searched four bytes at a time;
// at or behind `end`: there is none.  Bytes behind `nbytes` read as 0.
__device__ __forceinline__ u64 find_byte(const u8 *text, u64 i, u64 end, u64 nbytes, u32 four) {
  for (; i < end; i += 4) {
    const u32 z = zero_bytes(load_u32_unaligned(text, i, nbytes) ^ four);
    if (z) { i += (u32)(__ffs((int)z) - 1) >> 3; break; }
  }
  return i;
}
// where entry r of a window's newline-terminated entries begins and how long it is, from where each entry's newline lies; an
// index that does not fit the entries (the caller's *d_bad says so) gives an empty one
__device__ __forceinline__ void window_entry(const u64 *ent_end, u64 entry_bytes, u64 r, u64 *es, u64 *E) {
  const u64 s = r ? ent_end[r - 1] + 1 : 0, e = ent_end[r];
  const bool ok = s <= e && e < entry_bytes;
  *es = ok ? s : 0;
  *E = ok ? e - s : 0;
}

struct CommentArgs {
  const u8 *text;       // the piece
  u64 nbytes;
  const u64 *line_end;  // its line index
  u32 unit_lines;       // text lines per row: a record, or a pair under -i
  u32 line0;            // the header line of this mate inside the unit (0; mate 2 of an interleaved text: lines per record)
  u64 nrec;             // rows taken from the piece
  u64 row0;             // run-wide row of the first of them (error messages)
  const u8 *namelen;    // the piece's stored name lengths when the name pass ran for this mate, else null: scan for the space
  u16 *comlen;          // the piece's rows of the entry lengths
  u64 *off;             // nrec + 1: where each entry begins among the piece's, and their size
  u8 *dst;              // the store, from the piece's first byte on
  u32 *longest;         // the run's longest entry
  DevErr *err;
};
__device__ __forceinline__ void comment_line(const CommentArgs &a, u64 r, u64 *ns, u64 *p0) {
  const u64 line = (u64)a.unit_lines * r + a.line0;
  *ns = line ? a.line_end[line - 1] + 1 : 0;
  *p0 = a.line_end[line];
}
// one thread per row: the entry is the header line's tail from the first space on.  Behind the name pass its length is the
// line's minus '@' and the stored name; otherwise the line is searched for the space four bytes at a time.
__global__ __launch_bounds__(256) void comment_plan_k(CommentArgs a) {
  __shared__ u32 wg_max;
  if (threadIdx.x == 0) wg_max = 0;
  __syncthreads();
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.nrec) {
    u64 ns, p0;
    comment_line(a, r, &ns, &p0);
    u64 len = 0;
    if (p0 > ns) {  // (an empty header line is the name pass's error)
      const u64 body = p0 - ns - 1;  // behind '@'
      if (a.namelen) {
        len = body >= a.namelen[r] ? body - a.namelen[r] : 0;
      } else {
        const u64 i = find_byte(a.text, ns + 1, p0, a.nbytes, 0x20202020u);
        len = i < p0 ? p0 - i : 0;
      }
    }
    if (len > COM_MAX) {
      dev_fail(a.err, E_COMMENT, a.row0 + r, (u32)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull));
      len = 0;  // (the run ends with the error; until the host sees it the store must stay well-formed)
    }
    a.comlen[r] = (u16)len;
    if (len) atomicMax(&wg_max, (u32)len);
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_max) atomicMax(a.longest, wg_max);
}
struct CommentSize {  // an entry's bytes in the stream: with its newline
  const u16 *comlen;
  __device__ u64 operator()(u64 r) const { return (u64)comlen[r] + 1; }
};
// The entry and the newline behind it are ONE run of the text: the last comlen + 1 bytes of the header line, newline included.
// Entries are about a dozen bytes, so nearly every 16-byte granule of the store would meet a seam: a lane per destination byte
// instead (as in fastq_records_k) -- a wavefront's stores are 64 contiguous bytes, its loads the tails of a few neighbouring
// lines.  A workgroup owns COM_SPAN bytes and narrows the search for a byte's row to the rows its span meets.
__global__ __launch_bounds__(256) void comment_copy_k(CommentArgs a) {
  __shared__ u64 r_span[2];
  const u64 total = a.off[a.nrec];
  const u64 span0 = (u64)blockIdx.x * COM_SPAN;
  if (span0 >= total) return;
  const u64 span1 = span0 + COM_SPAN < total ? span0 + COM_SPAN : total;
  if (threadIdx.x < 2) r_span[threadIdx.x] = vl_record_of(a.off, 0, a.nrec, threadIdx.x ? span1 - 1 : span0);
  __syncthreads();
  const u64 r_lo = r_span[0], r_hi = r_span[1] + 1;
#pragma unroll 1
  for (u32 c = 0; c < COM_CHUNKS; c++) {
    const u64 x = span0 + (u64)c * 256u + threadIdx.x;
    if (x >= span1) break;
    const u64 r = vl_record_of(a.off, r_lo, r_hi, x);
    u64 ns, p0;
    comment_line(a, r, &ns, &p0);
    const u64 j = x - a.off[r], len = a.comlen[r];  // j <= len: every entry holds at least its newline
    a.dst[x] = j < len ? a.text[p0 - len + j] : (u8)'\n';
  }
}

// ---- decompress: insert -------------------------------------------------------------------------------------------------
struct InsertArgs {
  const u8 *text;        // a window's records (fastq_records_k): "@name\n" bases ["\n+\n" qualities] "\n"
  const u64 *rec_off;    // nrec + 1: where each begins, and the text's size
  const u8 *entries;     // the window's entries of the comment stream, each followed by its newline
  u64 entry_bytes;
  const u64 *ent_end;    // nrec: where each entry's newline lies in `entries` (a newline index made on the device)
  u64 tail[2];           // bytes from the header line's newline to the record's end: 2 L + 5 with qualities, L + 2 without;
  u32 par;               // record r takes tail[r & par]: 0, or 1 for an interleaved text (mate 1's records are the even ones)
  u64 nrec;
  u64 *dst_off;          // nrec + 1: the same for the text with the entries put in
  u8 *dst;
};
struct InsertedSize {
  InsertArgs a;
  __device__ u64 operator()(u64 r) const {
    u64 es, E;
    window_entry(a.ent_end, a.entry_bytes, r, &es, &E);
    return a.rec_off[r + 1] - a.rec_off[r] + E;
  }
};
// The mirror image of strip_copy_k: a record with its entry is three runs -- "@name" from the text, the entry from the window's
// entries, then the header line's newline and everything behind it from the text again.  The newline lies `tail` bytes in
// front of the record's end.
__global__ __launch_bounds__(256) void insert_copy_k(InsertArgs a) {
  __shared__ u64 r_span[2];
  const u64 total = a.dst_off[a.nrec], nsrc = a.rec_off[a.nrec];
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
    u64 d0, s0, nl, es, A, E, size;
    auto view = [&](u64 rr) {
      const u64 e = a.rec_off[rr + 1];
      d0 = a.dst_off[rr];
      s0 = a.rec_off[rr];
      const u64 tail = a.tail[rr & a.par];
      const u64 T = e - s0 < tail ? e - s0 : tail;  // (a record shorter than its tail: never reached in front of it)
      nl = e - T;                // the header line's newline
      A = nl - s0;               // '@' and the name
      window_entry(a.ent_end, a.entry_bytes, rr, &es, &E);  // the entry, without its newline
      size = A + E + T;
    };
    view(r);
    const u64 j0 = x0 - d0;
    if (x1 - x0 == 16 && j0 + 16 <= size) {
      if (j0 + 16 <= A) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, s0 + j0, nsrc); continue; }
      if (j0 >= A && j0 + 16 <= A + E) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.entries, es + (j0 - A), a.entry_bytes); continue; }
      if (j0 >= A + E) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, nl + (j0 - A - E), nsrc); continue; }
    }
    for (u64 x = x0; x < x1; x++) {
      while (x - d0 >= size) view(++r);  // (x < total: there is such a record)
      const u64 j = x - d0;
      a.dst[x] = j < A ? a.text[s0 + j] : j < A + E ? a.entries[es + (j - A)] : a.text[nl + (j - A - E)];
    }
  }
}
// An interleaved window: where each of its 2 n records begins, from where its n pairs begin -- mate 2's record is '@', its name
// (name_off2: where each of mate 2's name records, a length byte and the name, begins) and tail2 bytes in front of the pair's end
__global__ __launch_bounds__(256) void pair_split_k(u64 npairs, const u64 *pair_off, const u64 *name_off2, u64 tail2, u64 *rec_off) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > npairs) return;
  rec_off[2 * k] = pair_off[k];
  if (k == npairs) return;
  const u64 size2 = (name_off2[k + 1] - name_off2[k]) + tail2, e = pair_off[k + 1];
  rec_off[2 * k + 1] = e - pair_off[k] < size2 ? pair_off[k] : e - size2;
}
__global__ __launch_bounds__(256) void pair_offsets_k(u64 npairs, const u64 *rec_off, u64 *pair_off) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= npairs) pair_off[k] = rec_off[2 * k];
}
// *bad is set when the entries do not hold exactly nrec newlines, the last of them at their end
__global__ void insert_check_k(const u64 *nlines, const u8 *entries, u64 entry_bytes, u64 nrec, u32 *bad) {
  *bad = (*nlines != nrec || (entry_bytes && entries[entry_bytes - 1] != '\n')) ? 1u : 0u;
}

}  // namespace scalce
