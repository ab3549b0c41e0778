// archive_walk.hpp -- the streams of an archive as the decompress host (stream_decode.cpp) walks them: the headers, mate 1's
// buckets, and one function per stream that advances it by n records -- into a destination (a window's share of the slot's
// pinned block) or, in front of a range, to nowhere.  Host side only: callbacks, bytes that come from a file and a core table
// behind two lookups; no device call, no HIP header, so that the parser of untrusted input runs on its own
// (tools/archive_walk_check.cpp).  The walk runs on the session's main thread: a failure fills the Failure it is handed and
// comes back as its code; the session records it.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/scalce_hip.h"
#include "commentstream.hpp"
#include "lenstream.hpp"
#include "plusstream.hpp"
#include "stream_src.hpp"

namespace scalce_host {
typedef uint32_t u32;
constexpr u64 FRAME = SCALCE_AC_BLOCK;
constexpr u64 UNKNOWN = ~0ull;

struct Failure {
  int rc = SCALCE_OK;
  std::string msg;
  int mate = -1, stream = -1, wants_file = 0;
};
__attribute__((format(printf, 6, 7))) inline int failure(Failure &f, int rc, int mate, int stream, int wants_file, const char *fmt, ...) {
  char b[600];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  f.rc = rc; f.msg = b; f.mate = mate; f.stream = stream; f.wants_file = wants_file;
  return rc;
}
// the streams the walk names in a failure: r, n, q, l, o, c, x, p by the letter that ends their files' names.  The values reach
// the library's callers through Failure::stream (scalce_unpack_stats.error_stream): they stay as they are.
enum StreamId { ST_READ = 0, ST_NAME = 1, ST_QUALITY = 2, ST_LENGTH = 3, ST_ORDER = 4, ST_COMMENT = 5, ST_EXCEPTION = 6, ST_PLUS = 7 };
inline const char *stream_name(int stream) {
  static const char *const NAME[8] = {"read", "name", "quality", "length", "order", "comment", "exception", "plus-line"};
  return NAME[stream >= 0 && stream < 8 ? stream : ST_ORDER];
}
// a stream that ends, or fails, before what is asked of it
inline int read_error(Failure &f, int m, int stream) { return failure(f, SCALCE_ERR_FORMAT, m, stream, 0, "read error on the %s stream", stream_name(stream)); }
inline int truncated(Failure &f, int m, int stream) { return failure(f, SCALCE_ERR_FORMAT, m, stream, 0, "(ERROR) truncated %s stream", stream_name(stream)); }
inline int short_stream(Failure &f, int m, int stream, const Src &s) { return s.bad ? read_error(f, m, stream) : truncated(f, m, stream); }

// the core table, as far as a bucket header needs it (the session fills it from the context's patterns)
struct CoreTable {
  int count = 0;
  int (*length)(void *user, int core) = nullptr;
  const char *(*string)(void *user, int core) = nullptr;
  void *user = nullptr;
};

// mate 1's read stream: buckets, each opened by [i32 core][u64 records] (decompress.cpp:262-270).  The walk is serial -- a
// header tells how far the next one is -- and runs along with the stream as it arrives: no seek, so a gzip container will do.
struct Buckets {
  u64 left = 0;  // records of the current bucket not yet taken
  u32 core_len = 0, rec_bytes = 0;
  char core[32];
  u8 header[12];
};

// What the two streams of text entries -- one newline-terminated entry per record -- differ in on the walk: their id and the
// text of their failures, and what the plus-line stream alone has: a header whose longest entry is 0 says that no entries
// follow (every record's is the empty one), and an entry has to be of a class (plusstream.hpp).
struct TextKind {
  StreamId stream;
  const char *(*header_read)(const uint8_t *h, size_t have, uint32_t *longest, uint64_t *n);
  const char *(*entry_too_long)();
  int (*count_message)(char *out, size_t cap, uint64_t entries, uint64_t records);
  bool header_alone;                              // longest == 0: the file is its header
  const char *(*wrong)(const u8 *e, size_t len);  // what is wrong with an entry of len bytes, or nullptr
};
inline const char *any_entry(const u8 *, size_t) { return nullptr; }
inline const char *plus_entry_wrong(const u8 *e, size_t len) { return plus_class(e, len) == PLUS_MALFORMED ? plus_malformed() : nullptr; }
inline constexpr TextKind COMMENT_KIND = {ST_COMMENT, comment_header_read, comment_entry_too_long, comment_count_message, false, any_entry};
inline constexpr TextKind PLUS_KIND = {ST_PLUS, plus_header_read, plus_entry_too_long, plus_count_message, true, plus_entry_wrong};
static_assert(COMMENT_HEADER_BYTES == PLUS_HEADER_BYTES, "the text streams share a header");
// ... and such a stream of a mate, and where the walk stands in it
struct TextStream {
  const TextKind *kind;
  Src src;
  bool open = false;
  u32 longest = 0;          // its header's C or P: the longest entry, without the newline
  u64 total = 0, taken = 0;  // its header's N; entries taken or passed over so far
  u64 delivered = 0, skipped = 0;
  bool no_entries() const { return kind->header_alone && !longest; }
};

// what a mate's streams are and where the walk stands in them
struct ArcMate {
  Src r, n, q;
  Src l;                     // the length stream of a variable-length archive (params len_rd), or not open
  bool has_len = false;
  int l_width = 0;           // bytes per entry
  u64 l_delivered = 0, l_skipped = 0;
  TextStream com{&COMMENT_KIND};  // the comment stream of an archive made with --keep-comments (scalce_unpack_comments), or not open
  TextStream plus{&PLUS_KIND};    // the plus-line stream of an archive made with --keep-plus (scalce_unpack_plus), or not open
  int L = 0, no_ac = 0;
  int64_t phred = 0;
  bool q_empty = false;
  u64 total_syms = 0, records_left = UNKNOWN, first = 0;
  u64 range_left = UNKNOWN;  // records of the range not yet taken (UNKNOWN: the range runs to the archive's end)
  u64 drop = 0;              // symbols of the first batch that lie in front of the range's first record
  Buckets bk;
  u64 frames_left = 0, syms_left = 0;  // of the coded quality stream, not yet handed to the decoder
};

// where a window's share of a read stream goes: the slice and its bucket directory, what they hold, and what came into them
struct ReadsDst {
  u8 *slice; scalce_fq_bucket *dir; u64 cap_slice; u32 cap_dir;
  u64 bytes = 0;  // of the slice, inline headers included
  u32 ndir = 0;
};
// ... and a mate's names: the name records as they are, and where each begins (one entry more than there are names)
struct NamesDst { u8 *bytes; u64 *off; u64 cap; };
// ... and its entries of the comment stream, each with its newline, as the stream holds them
struct CommentsDst { u8 *bytes; u64 cap; u64 nbytes = 0; };
// ... and of the plus-line stream, the same; grow = what they add to the window's text
struct PlusDst { u8 *bytes; u64 cap; u64 nbytes = 0; u64 grow = 0; };

// The arithmetic of a range over the coded quality stream, without a device call: symbols [first * L, (first + n) * L) of a
// stream of total_syms symbols in frames of SCALCE_AC_BLOCK.  first and n are clamped to the total_syms / L records the stream
// holds; a range that reaches the last record takes the symbols behind it (fewer than one record) along, as a whole run does.
inline int range_plan_quality(int read_len, u64 first, u64 n, u64 total_syms, u64 out[4]) {
  if (read_len <= 0 || !out) return SCALCE_ERR_ARG;
  const u64 L = (u64)read_len, records = total_syms / L;
  first = std::min(first, records);
  n = std::min(n, records - first);
  const u64 s0 = first * L, s1 = first + n == records ? total_syms : (first + n) * L;
  out[0] = s0 / FRAME;
  out[1] = out[2] = out[3] = 0;
  if (!n) return SCALCE_OK;
  out[1] = (s1 + FRAME - 1) / FRAME - out[0];
  out[2] = s0 - out[0] * FRAME;
  out[3] = s1 - s0;
  return SCALCE_OK;
}

struct Walk {
  ArcMate *M[2] = {nullptr, nullptr};  // (the session's mates: each carries its device half behind this one)
  CoreTable cores;
  int m0 = 0, m1 = 0;  // the mates of the pass that runs (one mate, or both under -i)
  bool known = false;  // ... and whether a symbol count says how many records they hold
  bool names = false, qual = true;
  std::string library;

  // ---- headers (decompress.cpp:131-237) ------------------------------------------------------------------------------
  int headers(const scalce_unpack_params &P, const scalce_unpack_range &RG, scalce_read_fn rd[2][3], void *user[2][3], double *wait,
              scalce_unpack_range_stats &RS, Failure &f) {
    qual = !P.no_qualities;
    for (int m = 0; m < P.mates; m++) {
      ArcMate &x = *M[m];
      x.r.open(rd[m][0], RG.skip[m][0], user[m][0], wait, &RS.bytes_delivered[m][0], &RS.bytes_skipped[m][0]);
      x.n.open(rd[m][1], RG.skip[m][1], user[m][1], wait, &RS.bytes_delivered[m][1], &RS.bytes_skipped[m][1]);
      x.q.open(qual ? rd[m][2] : nullptr, RG.skip[m][2], qual ? user[m][2] : nullptr, wait, &RS.bytes_delivered[m][2], &RS.bytes_skipped[m][2]);
      if (!x.r.need(8) || memcmp(x.r.ptr(), "scalce2", 7)) return failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 1, "is not a scalce archive");
      const bool has_no_ac = x.r.ptr()[6] == '2' && x.r.ptr()[7] >= '2';
      x.r.skip(8);
      int32_t v = 0;
      if (has_no_ac) {
        if (!x.r.get(v)) return truncated(f, m, ST_READ);
        x.no_ac = v;
      }
      if (!x.r.get(v)) return truncated(f, m, ST_READ);
      x.L = v;
      if (x.L <= 0) return failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 0, "(ERROR) read length %d in the read stream's header", x.L);
      if (x.r.bad) return read_error(f, m, ST_READ);
      if (qual) {
        if (x.q.need(16)) { x.q.skip(8); x.q.get(x.phred); } else x.q.skip(x.q.avail());
        x.q_empty = !x.q.need(1);
        if (x.q.bad) return read_error(f, m, ST_QUALITY);
      }
      if (x.n.need(8)) x.n.skip(8);
      if (P.len_rd[m]) {  // the fourth stream: header, then one entry per record
        x.l.open(P.len_rd[m], P.len_skip[m], P.len_user[m], wait, &x.l_delivered, &x.l_skipped);
        int hl = 0;
        const bool whole = x.l.need(LEN_HEADER_BYTES);
        if (x.l.bad) return read_error(f, m, ST_LENGTH);
        if (const char *why = len_header_read(x.l.ptr(), whole ? LEN_HEADER_BYTES : 0, &x.l_width, &hl)) return failure(f, SCALCE_ERR_FORMAT, m, ST_LENGTH, 0, "(ERROR) %s", why);
        x.l.skip(LEN_HEADER_BYTES);
        if (hl != x.L)
          return failure(f, SCALCE_ERR_FORMAT, m, ST_LENGTH, 0, "(ERROR) the length stream was written for reads of up to %d bases, the read stream holds reads of %d", hl, x.L);
        x.has_len = true;
      }
    }
    if (P.ignore_names) {
      library = P.library ? P.library : "";
    } else {
      u8 nm = 0;
      for (int m = 0; m < P.mates; m++) M[m]->n.get(nm);
      names = nm != 0;
      if (!names)
        for (int m = 0; m < P.mates; m++) {  // int64 0, then the library name to the end of the stream
          Src &n = M[m]->n;
          if (n.need(8)) n.skip(8);
          library.clear();
          while (n.need(1)) { library.append((const char *)n.ptr(), n.avail()); n.skip(n.avail()); if (library.size() > 4096) break; }
        }
    }
    if (!names && library.size() > 255) return failure(f, SCALCE_ERR_ARG, -1, ST_NAME, 0, "library name longer than 255 characters");
    if (P.interleave && M[0]->no_ac != M[1]->no_ac) return failure(f, SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) the mates were not archived together");
    return SCALCE_OK;
  }

  // ---- mate 1's buckets ----------------------------------------------------------------------------------------------
  // moves to the next bucket that has records; 0: there is one, 1: the stream has ended, < 0: failed
  int next_bucket(int m, Failure &f, size_t look = ~(size_t)0) {
    ArcMate &x = *M[m];
    while (!x.bk.left) {
      if (!x.r.need(12, look)) {
        if (x.r.bad) { read_error(f, m, ST_READ); return -1; }
        return 1;
      }
      int32_t core = 0;
      u64 cnt = 0;
      memcpy(x.bk.header, x.r.ptr(), 12);
      x.r.get(core);
      x.r.get(cnt);
      x.bk.core_len = 0;
      if (core != SCALCE_ROOT_CORE) {
        const bool has = core >= 0 && core < cores.count;
        const int cl = has ? cores.length(cores.user, core) : -1;
        const char *cs = has ? cores.string(cores.user, core) : nullptr;
        if (cl < 0 || !cs) {
          failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 0, "(ERROR) archive refers to core %d which the core table does not have", core);
          return -1;
        }
        if (cl > (int)sizeof x.bk.core || cl > x.L) { failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 0, "(ERROR) core %d does not fit the reads", core); return -1; }
        x.bk.core_len = (u32)cl;
        memcpy(x.bk.core, cs, (size_t)cl);
      }
      x.bk.rec_bytes = (u32)((x.L - (int)x.bk.core_len + 3) / 4) + (x.L > 255 ? 2u : 1u);
      x.bk.left = cnt;
    }
    return 0;
  }

  // ---- which stream says how many records there are ---------------------------------------------------------------------
  // Where no symbol count says how many records the archive holds (`known`), the streams that end it for a whole run -- the
  // names, else the raw quality rows, else the read stream, of the pass's first mate -- end it in front of a range too: a
  // range that begins behind them is empty.  A short read on the stream that decides (r, n or q) ends the archive and is
  // no error; any other stream (l never decides) that ends in front of the range, or inside a window, is truncated.
  bool decides_count(int m, int stream) const {
    if (known || m != m0 || stream > ST_QUALITY) return false;
    return stream == ST_NAME || (!names && (stream == ST_QUALITY || !(qual && M[m]->no_ac)));
  }
  // ... applied: a stream gave `got` whole records of the n asked for -- n shrinks, or the stream is truncated
  int ended_at(int m, int stream, u64 got, u64 &n, Failure &f) const {
    if (got != n && !decides_count(m, stream)) return truncated(f, m, stream);
    n = got;
    return SCALCE_OK;
  }
  // does mate m's read stream hold another record (mate 2, which has no headers: another `least` bytes)?
  int more_reads(int m, size_t least, bool &more, Failure &f) {
    if (m != 0) { more = M[m]->r.need(least); return SCALCE_OK; }
    const int e = next_bucket(0, f);
    more = e == 0;
    return e < 0 ? f.rc : SCALCE_OK;
  }
  // What a window is measured in: bytes of FASTQ text, four lines per record, whether or not the archive holds qualities.
  // The two-line records of -Q / -f are cut at the same records as their FASTQ would be, so the records per window -- and
  // with them every buffer -- depend on the window and the read length alone.
  u64 rec_budget(int m) const { return 2ull * (u64)M[m]->L + 6; }

  // ---- a stream moves on by n records: into `to`, or -- without one -- passed over ----------------------------------------
  // Passed over, nothing reaches the caller: the bytes go through Src::pass (the caller's skip, or reads that are dropped).
  // got = the whole records the stream gave; fewer than n is for the caller to judge (ended_at), a stream that fails or ends
  // inside a record is a failure here.
  // The read stream.  Mate 1's goes bucket by bucket: every header is read and checked; the directory gets an entry per
  // bucket that has records in the window, and headers inside the slice stay inline
  int reads(int m, u64 n, ReadsDst *to, u64 &got, Failure &f) {
    constexpr size_t LOOK = 64u << 10;  // read ahead of a bucket header when the bucket behind it is skipped, not read
    ArcMate &x = *M[m];
    got = 0;
    if (m != 0) {  // bare records in mate 1's order
      const u64 rb = (u64)(x.L + 3) / 4;
      const u64 bytes = to ? x.r.read_into(to->slice, n * rb) : x.r.pass(n * rb);
      if (x.r.bad) return read_error(f, m, ST_READ);
      got = bytes / rb;
      if (bytes % rb) return truncated(f, m, ST_READ);
      if (to) {
        memset(&to->dir[0], 0, sizeof to->dir[0]);
        to->dir[0].rec_bytes = (u32)rb;
        to->ndir = 1; to->bytes = bytes;
      }
      return SCALCE_OK;
    }
    while (got < n) {
      if (!x.bk.left) {
        const int e = next_bucket(m, f, !to && x.r.skp ? LOOK : ~(size_t)0);
        if (e < 0) return f.rc;
        if (e) break;
        if (to && got) { memcpy(to->slice + to->bytes, x.bk.header, 12); to->bytes += 12; }  // headers inside the slice stay inline
      }
      const u64 t = std::min(x.bk.left, n - got), bytes = t * x.bk.rec_bytes;
      if (!to) {
        if (x.r.pass(bytes) != bytes) return short_stream(f, m, ST_READ, x.r);
      } else {
        if (to->ndir == to->cap_dir || to->bytes + bytes > to->cap_slice)
          return failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 0, "(ERROR) the read stream opens more buckets than the core table has cores");
        if (x.r.read_into(to->slice + to->bytes, bytes) != bytes) return short_stream(f, m, ST_READ, x.r);
        scalce_fq_bucket &b = to->dir[to->ndir++];
        memset(&b, 0, sizeof b);
        b.first = got; b.off = to->bytes; b.core_len = x.bk.core_len; b.rec_bytes = x.bk.rec_bytes;
        memcpy(b.core, x.bk.core, x.bk.core_len);
        to->bytes += bytes;
      }
      got += t; x.bk.left -= t;
    }
    return SCALCE_OK;
  }
  // n records of `width` bytes each (-A: the q - offset rows of L bytes as they are; the length stream: entries of one width)
  int rows(int m, int stream, Src &s, u64 width, u64 n, u8 *to, u64 &got, Failure &f) {
    const u64 bytes = to ? s.read_into(to, n * width) : s.pass(n * width);
    if (s.bad) return read_error(f, m, stream);
    got = bytes / width;
    return bytes % width ? truncated(f, m, stream) : SCALCE_OK;
  }
  int quality_rows(int m, u64 n, u8 *to, u64 &got, Failure &f) { return rows(m, ST_QUALITY, M[m]->q, (u64)M[m]->L, n, to, got, f); }
  int lengths(int m, u64 n, u8 *to, u64 &got, Failure &f) { return rows(m, ST_LENGTH, M[m]->l, (u64)M[m]->l_width, n, to, got, f); }
  // names in front of a range: a length byte per name has to be read, so they go through the look-ahead buffer, not through skip
  int pass_names(int m, u64 n, u64 &got, Failure &f) {
    Src &src = M[m]->n;
    for (got = 0; got < n && src.need(1); got++) {
      const size_t len = src.ptr()[0];
      if (!src.need(1 + len)) return short_stream(f, m, ST_NAME, src);
      src.skip(1 + len);
    }
    return src.bad ? read_error(f, m, ST_NAME) : SCALCE_OK;
  }
  // ---- the text-entry streams (commentstream.hpp, plusstream.hpp): a fifth and a sixth cursor of the mate, walked alike ----
  int text_open(int m, TextStream &t, scalce_read_fn rd, void *user, double *wait, Failure &f) {
    const int id = t.kind->stream;
    t.src.open(rd, nullptr, user, wait, &t.delivered, &t.skipped);
    const bool whole = t.src.need(COMMENT_HEADER_BYTES);
    if (t.src.bad) return read_error(f, m, id);
    if (const char *why = t.kind->header_read(t.src.ptr(), whole ? COMMENT_HEADER_BYTES : 0, &t.longest, &t.total))
      return failure(f, SCALCE_ERR_FORMAT, m, id, 0, "(ERROR) %s", why);
    t.src.skip(COMMENT_HEADER_BYTES);
    t.open = true;
    t.taken = 0;
    return SCALCE_OK;
  }
  // the next entry where it lies in the look-ahead buffer: at = its bytes, len = how many with the newline.  0: there it is; 1:
  // the stream ends here, between two entries; else the failure -- it ends inside an entry, an entry outgrows the header's
  // longest or is none of its kind, a read failed.  A stream that is its header alone holds no entries: every record's is the
  // empty one.
  int next_text(int m, TextStream &t, const u8 *&at, size_t &len, Failure &f) {
    static const u8 bare[1] = {'\n'};
    const int id = t.kind->stream;
    if (t.no_entries()) {
      if (t.taken >= t.total) return 1;
      at = bare; len = 1;
      return 0;
    }
    Src &c = t.src;
    size_t seen = 0;
    for (;;) {
      const size_t have = c.avail();
      if (have > seen) {
        const void *nl = memchr(c.ptr() + seen, '\n', have - seen);
        if (nl) {
          len = (size_t)((const u8 *)nl - c.ptr()) + 1;
          if (len - 1 > t.longest) return failure(f, SCALCE_ERR_FORMAT, m, id, 0, "(ERROR) %s", t.kind->entry_too_long());
          at = c.ptr();
          if (const char *why = t.kind->wrong(at, len - 1)) return failure(f, SCALCE_ERR_FORMAT, m, id, 0, "(ERROR) %s", why);
          return 0;
        }
        seen = have;
      }
      if (seen > t.longest) return failure(f, SCALCE_ERR_FORMAT, m, id, 0, "(ERROR) %s", t.kind->entry_too_long());
      if (!c.need(seen + 1)) {
        if (c.bad) return read_error(f, m, id);
        return seen ? truncated(f, m, id) : 1;
      }
    }
  }
  void text_taken(TextStream &t, size_t len) {
    if (!t.no_entries()) t.src.skip(len);
    t.taken++;
  }
  // entries in front of a range: passed over on the host by their newlines (a stream that holds entries is always read, as
  // the names are); none behind the range is read
  int pass_text(int m, TextStream &t, u64 n, u64 &got, Failure &f) {
    for (got = 0; got < n; got++) {
      const u8 *at;
      size_t len = 0;
      const int e = next_text(m, t, at, len, f);
      if (e == 1) break;
      if (e) return e;
      text_taken(t, len);
    }
    return SCALCE_OK;
  }
  int text_count(int m, const TextStream &t, u64 entries, u64 records, Failure &f) const {
    char b[200];
    t.kind->count_message(b, sizeof b, entries, records);
    return failure(f, SCALCE_ERR_FORMAT, m, t.kind->stream, 0, "(ERROR) %s", b);
  }
  // the plus-line stream's next entry with its class
  int next_plus(int m, const u8 *&at, size_t &len, PlusClass &cls, Failure &f) {
    const int e = next_text(m, M[m]->plus, at, len, f);
    if (!e) cls = plus_class(at, len - 1);
    return e;
  }
  // One record's (pair's) entries into `to`, if they and what they add fit: header[i] = the bytes of mate i's header line behind
  // its '@' as this run writes it, which is what a repeat adds.  grow = what the entries add to the text.  0: peeked (nothing is
  // consumed before plus_commit); 1: mate 1's stream ends here, between two entries; else the failure.
  struct PlusPeek { const u8 *at[2]; size_t len[2] = {0, 0}; PlusClass cls[2] = {PLUS_BARE, PLUS_BARE}; u64 grow = 0; };
  int plus_peek(const u64 header[2], PlusPeek &k, Failure &f) {
    k.grow = 0;
    for (int i = 0; i <= m1 - m0; i++) {
      const int e = next_plus(m0 + i, k.at[i], k.len[i], k.cls[i], f);
      if (e == 1 && i) return truncated(f, m0 + i, ST_PLUS);
      if (e) return e;
      k.grow += plus_growth(k.cls[i], k.len[i] - 1, header[i]);
    }
    return SCALCE_OK;
  }
  bool plus_fits(const PlusDst &to, const PlusPeek &k) const { return to.nbytes + k.len[0] + k.len[1] <= to.cap; }
  void plus_commit(PlusDst &to, const PlusPeek &k) {
    for (int i = 0; i <= m1 - m0; i++) {
      memcpy(to.bytes + to.nbytes, k.at[i], k.len[i]);
      to.nbytes += k.len[i];
      text_taken(M[m0 + i]->plus, k.len[i]);
    }
    to.grow += k.grow;
  }

  // names of up to `ncap` records (pairs) of the pass's mates into to[], as many as W bytes of text take; n = how many.
  // com: each record's entry of the comment stream is taken in the same step and counts in the budget (two mates in one window:
  // mate 1's entry, then mate 2's, pair by pair -- the order of the records in the interleaved text)
  // plus: the same for each record's entry of the plus-line stream, with what it adds to the record's text
  int take_names(NamesDst to[2], u64 ncap, u64 W, u64 &n, u64 nb[2], Failure &f, CommentsDst *com = nullptr, PlusDst *plus = nullptr) {
    u64 text = 0;
    nb[0] = nb[1] = 0;
    n = 0;
    const int nmates = m1 - m0 + 1;
    while (n < ncap) {
      u32 len[2] = {0, 0};
      int ended = 0;
      u64 rec = 0;
      for (int i = 0; i < nmates; i++) {
        Src &src = M[m0 + i]->n;
        if (!src.need(1)) { ended++; continue; }
        len[i] = src.ptr()[0];
        if (!src.need(1 + (size_t)len[i])) return truncated(f, m0 + i, ST_NAME);
        rec += len[i] + rec_budget(m0 + i);
      }
      const u8 *cat[2] = {nullptr, nullptr};
      size_t clen[2] = {0, 0};  // the records' entries with their newlines
      for (int i = 0; i < nmates && com && !ended; i++) {
        const int e = next_text(m0 + i, M[m0 + i]->com, cat[i], clen[i], f);
        if (e == 1) return truncated(f, m0 + i, ST_COMMENT);
        if (e) return e;
        rec += clen[i] - 1;
      }
      PlusPeek pk;
      if (plus && !ended) {
        const u64 header[2] = {len[0] + (clen[0] ? clen[0] - 1 : 0), len[1] + (clen[1] ? clen[1] - 1 : 0)};
        if (const int e = plus_peek(header, pk, f)) return e == 1 ? truncated(f, m0, ST_PLUS) : e;
        rec += pk.grow;
      }
      if (ended) {
        for (int i = 0; i < nmates; i++) if (M[m0 + i]->n.bad) return read_error(f, m0 + i, ST_NAME);
        if (!decides_count(m0, ST_NAME) || ended != nmates) return truncated(f, m0, ST_NAME);
        break;
      }
      if (n && text + rec > W) break;
      bool fits = true;
      for (int i = 0; i < nmates; i++) fits = fits && nb[i] + 1 + len[i] <= to[i].cap;
      if (com) fits = fits && com->nbytes + clen[0] + clen[1] <= com->cap;
      if (plus) fits = fits && plus_fits(*plus, pk);
      if (!fits) break;
      if (plus) plus_commit(*plus, pk);
      for (int i = 0; i < nmates && com; i++) {
        memcpy(com->bytes + com->nbytes, cat[i], clen[i]);
        text_taken(M[m0 + i]->com, clen[i]);
        com->nbytes += clen[i];
      }
      for (int i = 0; i < nmates; i++) {
        Src &src = M[m0 + i]->n;
        to[i].off[n] = nb[i];
        memcpy(to[i].bytes + nb[i], src.ptr(), 1 + (size_t)len[i]);
        src.skip(1 + (size_t)len[i]);
        nb[i] += 1 + len[i];
      }
      text += rec;
      n++;
    }
    for (int i = 0; i < nmates; i++) to[i].off[n] = nb[i];
    return SCALCE_OK;
  }
  // coded qualities in front of a range: whole frames by their size words (no read ahead of a word whose frame is skipped)
  int pass_frames(int m, u64 frames, Failure &f) {
    Src &q = M[m]->q;
    for (u64 k = 0; k < frames; k++) {
      u32 sz = 0;
      if (!q.get(sz, q.skp ? 0 : ~(size_t)0) || q.pass(sz) != sz) return short_stream(f, m, ST_QUALITY, q);
    }
    return SCALCE_OK;
  }

  // What is left of the read streams holds no record -- where the range ends with the archive: behind a range that ends
  // sooner nothing is read, and a stream that is cut short there is not noticed.  more = the first mate that holds one, or -1
  int reads_at_end(int &more, Failure &f) {
    more = -1;
    if (M[m0]->range_left == 0 && M[m0]->records_left != 0) return SCALCE_OK;
    for (int m = m0; m <= m1 && more < 0; m++) {
      bool has = false;
      if (int rc = more_reads(m, (size_t)(M[m]->L + 3) / 4, has, f)) return rc;
      if (has) more = m;
    }
    return SCALCE_OK;
  }
  int holds_more(int m, Failure &f) const {
    return failure(f, SCALCE_ERR_FORMAT, m, ST_READ, 0, "(ERROR) the read stream holds more than the %llu records of the %s stream",
                   (unsigned long long)M[m]->first, names ? "name" : "quality");
  }
};

}  // namespace scalce_host
