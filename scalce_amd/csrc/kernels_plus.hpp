// kernels_plus.hpp -- the third line of a FASTQ record (--keep-plus).  The reference writes it back as a bare '+'; what stood
// behind the '+' goes into a stream of its own (PREFIX_<m>.scalcep), one newline-terminated ENTRY per record in archive order:
// empty for a bare '+', the byte '=' when the line repeats the header line (everything behind '@', name and what follows it),
// else '\'' and the line's bytes behind the '+'.  Compress side: per piece a plan pass (class and stored length per row, u16)
// and an extract pass (the entries, each with its class byte and its newline, appended to a per-mate byte store in input order);
// the emit stage gathers the store through the permutation with permute_copy_k (kernels_restore.hpp), as it gathers comments.
// Decompress side: a plan pass finds every record's '+' and its new size, a copy pass writes the text with the lines put back.
// It runs BEHIND strip_copy_k and insert_copy_k, which both assume the three bytes "\n+\n" between bases and qualities.
#pragma once
#include "kernels_comments.hpp"

namespace scalce {

constexpr u32 PLUS_MAX = 65535;  // the longest stored entry, class byte included (its length is a u16 row)
constexpr u8 PLUS_REPEAT = '=', PLUS_LITERAL = '\'';

// (CommentArgs carries the piece, its line index, unit_lines and line0; comlen holds the stored entry lengths here)
__device__ __forceinline__ void plus_lines(const CommentArgs &a, u64 r, u64 *hs, u64 *he, u64 *ls, u64 *le) {
  const u64 line = (u64)a.unit_lines * r + a.line0;
  *hs = line ? a.line_end[line - 1] + 1 : 0;
  *he = a.line_end[line];
  *ls = a.line_end[line + 1] + 1;
  *le = a.line_end[line + 2];
}
// one thread per row: bare, repeat or literal.  A repeat is found by the lengths first; only equal lengths are compared, four
// bytes at a time.  The stored length is 0 (bare), 1 (repeat) or 1 + the bytes behind the '+' (literal).
__global__ __launch_bounds__(256) void plus_plan_k(CommentArgs a) {
  __shared__ u32 wg_max;
  if (threadIdx.x == 0) wg_max = 0;
  __syncthreads();
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.nrec) {
    u64 hs, he, ls, le;
    plus_lines(a, r, &hs, &he, &ls, &le);
    u64 len = 0;
    if (le <= ls || a.text[ls] != '+') {
      dev_fail(a.err, E_PLUSLINE, a.row0 + r);
    } else if (le - ls > 1) {
      const u64 body = le - ls - 1;  // behind '+'
      bool same = he > hs && he - hs - 1 == body;
      for (u64 i = 0; same && i < body; i += 4) {
        u32 x = load_u32_unaligned(a.text, ls + 1 + i, a.nbytes) ^ load_u32_unaligned(a.text, hs + 1 + i, a.nbytes);
        if (body - i < 4) x &= (1u << (8 * (u32)(body - i))) - 1u;
        same = x == 0;
      }
      len = same ? 1 : body + 1;
      if (len > PLUS_MAX) {
        dev_fail(a.err, E_PLUSLONG, a.row0 + r, (u32)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull));
        len = 0;  // (the run ends with the error; until the host sees it the store must stay well-formed)
      }
    }
    a.comlen[r] = (u16)len;
    if (len) atomicMax(&wg_max, (u32)len);
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_max) atomicMax(a.longest, wg_max);
}
// A lane per destination byte, as in comment_copy_k and for the same reason: a repeat is two bytes, a bare line one, so nearly
// every 16-byte granule of the store would meet a seam.  Byte 0 of an entry is its class, its last byte the newline; the bytes
// between them are the third line's behind the '+'.
__global__ __launch_bounds__(256) void plus_copy_k(CommentArgs a) {
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
    const u64 j = x - a.off[r], len = a.comlen[r];  // j <= len: every entry holds at least its newline
    u8 ch = '\n';
    if (j < len) {
      if (j == 0) ch = len == 1 ? PLUS_REPEAT : PLUS_LITERAL;  // (a literal holds at least one byte behind its class)
      else {
        u64 hs, he, ls, le;
        plus_lines(a, r, &hs, &he, &ls, &le);
        ch = a.text[ls + j];
      }
    }
    a.dst[x] = ch;
  }
}
// how many rows hold a repeat (stored length 1) and a literal (longer), for the log: LDS first, one atomic pair per workgroup
__global__ __launch_bounds__(256) void plus_count_k(u64 n, const u16 *len, u32 *classes) {
  __shared__ u32 cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 l = r < n ? len[r] : 0;
  const u64 rep = __ballot(l == 1), lit = __ballot(l > 1);
  if ((threadIdx.x & 63) == 0) {
    if (rep) atomicAdd(&cnt[0], (u32)__popcll(rep));
    if (lit) atomicAdd(&cnt[1], (u32)__popcll(lit));
  }
  __syncthreads();
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&classes[threadIdx.x], cnt[threadIdx.x]);
}

// ---- decompress: the lines back -------------------------------------------------------------------------------------------
struct PlusArgs {
  const u8 *text;        // a window's records as the passes in front left them: "@header\n" bases "\n+\n" qualities "\n"
  const u64 *rec_off;    // nrec + 1: where each begins, and the text's size
  const u8 *entries;     // the window's entries of the plus-line stream, each followed by its newline
  u64 entry_bytes;
  const u64 *ent_end;    // nrec: where each entry's newline lies in `entries` (a newline index made on the device)
  u64 nrec;
  u64 *plus_at;          // nrec: where the record's '+' lies in `text`
  u64 *dst_off;          // nrec + 1: plus_insert_plan_k leaves the records' new sizes, the scan where each begins
  u8 *dst;
  u64 dst_cap;           // room in dst: a text that would outgrow it is not written (*bad)
  u32 *bad;
};
// One thread per record.  The header line's newline is searched forward from the record's start, four bytes at a time; with
// H bytes of header line the record is H + 2 l + 5 bytes, which says where the '+' lies.  A repeat grows the record by H - 1,
// a literal by its bytes behind the class byte.  A malformed entry (or a record that is no such text) sets *bad and adds nothing.
__global__ __launch_bounds__(256) void plus_insert_plan_k(PlusArgs a) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrec) return;
  const u64 s0 = a.rec_off[r], e = a.rec_off[r + 1], nsrc = a.rec_off[a.nrec];
  const u64 size = e >= s0 ? e - s0 : 0;
  const u64 i = find_byte(a.text, s0, e, nsrc, 0x0A0A0A0Au);
  const u64 H = i < e ? i - s0 : size;
  u64 es, E;
  window_entry(a.ent_end, a.entry_bytes, r, &es, &E);
  u64 grow = 0, at = s0;
  bool bad = false;
  if (H < 1 || size < H + 5 || ((size - H - 5) & 1)) {
    bad = E != 0;
  } else {
    at = s0 + H + 1 + (size - H - 5) / 2 + 1;
    if (E) {
      const u8 cls = a.entries[es];
      if (cls == PLUS_REPEAT && E == 1) grow = H - 1;
      else if (cls == PLUS_LITERAL && E > 1) grow = E - 1;
      else bad = true;
    }
  }
  a.plus_at[r] = at;
  a.dst_off[r] = size + grow;
  if (bad) *a.bad = 1u;
}
// The shape of insert_copy_k: 16-byte granules of the destination, seams byte by byte.  A record is three runs -- the text up
// to and including the '+', the inserted bytes (from the record's own header line behind '@' for a repeat, from the window's
// entries behind the class byte for a literal), the rest of the text.
__global__ __launch_bounds__(256) void plus_insert_copy_k(PlusArgs a) {
  __shared__ u64 r_span[2];
  const u64 total = a.dst_off[a.nrec], nsrc = a.rec_off[a.nrec];
  if (total > a.dst_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.bad = 1u;
    return;
  }
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
    u64 d0, s0, A, G, size, rest;
    const u8 *ins;      // what the inserted bytes are taken from: the text or the entries ...
    u64 ins_at, ins_n;  // ... where they begin in it, and its size (loads past it read 0)
    auto view = [&](u64 rr) {
      const u64 e = a.rec_off[rr + 1];
      d0 = a.dst_off[rr];
      s0 = a.rec_off[rr];
      size = a.dst_off[rr + 1] - d0;
      G = size - (e - s0);
      rest = a.plus_at[rr] + 1;  // behind the '+'
      A = rest - s0;
      ins = a.text; ins_at = s0 + 1; ins_n = nsrc;
      if (G) {
        u64 es, E;
        window_entry(a.ent_end, a.entry_bytes, rr, &es, &E);
        if (a.entries[es] == PLUS_LITERAL) { ins = a.entries; ins_at = es + 1; ins_n = a.entry_bytes; }
      }
    };
    view(r);
    const u64 j0 = x0 - d0;
    if (x1 - x0 == 16 && j0 + 16 <= size) {
      if (j0 + 16 <= A) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, s0 + j0, nsrc); continue; }
      if (j0 >= A && j0 + 16 <= A + G) {
        *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(ins, ins_at + (j0 - A), ins_n);
        continue;
      }
      if (j0 >= A + G) { *reinterpret_cast<uint4 *>(a.dst + x0) = vl_load16(a.text, rest + (j0 - A - G), nsrc); continue; }
    }
    for (u64 x = x0; x < x1; x++) {
      while (x - d0 >= size) view(++r);  // (x < total: there is such a record)
      const u64 j = x - d0;
      a.dst[x] = j < A ? a.text[s0 + j] : j < A + G ? ins[ins_at + (j - A)] : a.text[rest + (j - A - G)];
    }
  }
}
// An interleaved window after the passes in front: where each of its 2 n records begins, from where its n pairs begin.  Mate
// 1's record is its header line (searched forward, as above) and 2 l1 + 5 bytes.
__global__ __launch_bounds__(256) void plus_pair_split_k(u64 npairs, const u8 *text, const u64 *pair_off, u64 l1, u64 *rec_off) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > npairs) return;
  rec_off[2 * k] = pair_off[k];
  if (k == npairs) return;
  const u64 s0 = pair_off[k], e = pair_off[k + 1], nsrc = pair_off[npairs];
  const u64 i = find_byte(text, s0, e, nsrc, 0x0A0A0A0Au);
  const u64 size1 = (i < e ? i - s0 : 0) + 2 * l1 + 5;
  rec_off[2 * k + 1] = e - s0 < size1 ? s0 : s0 + size1;
}

}  // namespace scalce
