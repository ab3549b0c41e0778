// stream_decode.cpp -- streaming host of the decompress path: archives of any size through one GPU.
//
// What it replaces in the reference: the record loop of decompress.cpp:240-366, which reads one record of each stream at
// a time.  Here the archive moves through the device in WINDOWS of whole records: the three streams of a mate are read
// incrementally (scalce_read_fn), a window's slice of the read stream, its names and its bucket directory go up from
// pinned memory, fastq_records_k turns them into the window's text, the text comes down into pinned memory and is handed
// to the caller's write callback by a thread of its own.  Two sets of window buffers: while window w is on the device,
// window w + 1 is read and uploaded and window w - 1 is downloaded and written.
//
// Symbols and records do not share boundaries (a frame of the arithmetic coder holds SCALCE_AC_BLOCK symbols, no multiple
// of the read length): the coded quality stream is decoded in BATCHES of whole frames, ahead of the windows, on a stream
// of its own into one of two symbol buffers; windows consume whole records from the batch, and the rest of a batch --
// less than one record -- is carried in front of the next batch's symbols.  A wave decodes a frame as one serial chain,
// so a batch holds SCALCE_DECODE_AHEAD windows' worth of frames: the decoder's parallelism does not shrink with the window.
//
// Every buffer is sized from the window, the read length and the core table (DESIGN.md gives the formula), none from the
// archive; nothing is allocated or freed per window.
//
// A RANGE of records (scalce_stream_decompress_range; a whole run is the range from record 0 to the end) goes through the same
// window loop.  Before the first window, pass_over() moves every stream to the range's first record without handing a byte
// to the device: bucket headers are hopped, mate 2's records, raw quality rows and whole coded frames are skipped (the
// caller's skip, or reads that are dropped), names are hopped by their length bytes.  The decoder starts at the frame that
// holds the range's first symbol; the symbols of that frame in front of the record are decoded -- a frame is one chain -- and
// left in front of the first window's; the last frame of the range is launched for the symbols up to the range's end.
// Nothing behind the range is read: a stream that is cut short there is NOT noticed, and the check that the read streams
// hold no more records than the others is made only where the range ends with the archive.
//
// Built on the public C ABI only (include/scalce_hip.h) plus the HIP runtime for pinned memory, copies and events.
#include <hip/hip_runtime_api.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/scalce_hip.h"
#include "hip_own.hpp"
#include "lenstream.hpp"
#include "orderstream.hpp"
#include "stream_src.hpp"

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
using scalce_host::now_s;
using scalce_host::Src;

constexpr u64 FRAME = SCALCE_AC_BLOCK;
constexpr u64 TABLE_BYTES = 512000ull * 4;
constexpr u64 SCALCE_DECODE_AHEAD = 8;  // windows' worth of symbols per decoder batch
constexpr u64 UNKNOWN = ~0ull;

u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

struct Failure {
  int rc = SCALCE_OK;
  std::string msg;
  int mate = -1, stream = -1, wants_file = 0;
};

// mate 1's read stream: buckets, each opened by [i32 core][u64 records] (decompress.cpp:262-270).  The walk is serial -- a
// header tells how far the next one is -- and runs along with the stream as it arrives: no seek, so a gzip container will do.
struct Buckets {
  u64 left = 0;  // records of the current bucket not yet taken
  u32 core_len = 0, rec_bytes = 0;
  char core[32];
  u8 header[12];
};

// the arithmetic decoder of one mate: batches of whole frames ahead of the windows.  Everything here is made by
// setup_decoder() and goes with free_decoder(); the stream cursors and the window offsets are the Mate's
struct AcDecoderDelete { void operator()(scalce_ac_decoder *d) const { scalce_ac_decoder_destroy(d); } };
struct Decoder {
  std::unique_ptr<scalce_ac_decoder, AcDecoderDelete> dec;
  u64 G = 0, ycap = 0, coded_cap = 0;
  DBuf Y[2], d_coded[2], d_off[2];
  DBuf d_size[2];  // G sizes and the walk's verdict behind them
  HBuf h_coded;
  HBuf h_bad;      // one word per parity
  Event ev_coded_up, ev_dec[2], ev_rec[2], t_dec0[2], t_dec1[2];
  bool coded_up_once = false, rec_once[2] = {false, false};
  u64 have_b[2] = {0, 0};     // symbols a batch buffer holds, carry included
  int64_t enq = -1, cur = -1;  // last batch enqueued, batch being consumed
  u64 pos = 0;                // consumed of the current batch
};

struct Mate {
  Src r, n, q;
  Src l;                     // the length stream of a variable-length archive (params len_rd), or not open
  bool has_len = false;
  int l_width = 0;           // bytes per entry
  u64 l_delivered = 0, l_skipped = 0;
  int L = 0, no_ac = 0;
  int64_t phred = 0;
  bool q_empty = false;
  u64 total_syms = 0, records_left = UNKNOWN, first = 0;
  u64 range_left = UNKNOWN;  // records of the range not yet taken (UNKNOWN: the range runs to the archive's end)
  u64 drop = 0;              // symbols of the first batch that lie in front of the range's first record
  Buckets bk;
  u64 frames_left = 0, syms_left = 0;  // of the coded quality stream, not yet handed to the decoder
  Decoder d;
  // where this mate's parts of a window lie in the slot's input block
  u64 o_reads = 0, o_dir = 0, o_names = 0, o_noff = 0, o_qual = 0;
  u64 cap_slice = 0, cap_names = 0;
};

struct Slot {
  HBuf h_in, h_text, h_roff;
  DBuf d_in, d_text, d_roff;
  // variable-length archives: the window's entries of the length stream, and what strips the pad off its text
  HBuf h_len;
  DBuf d_len, d_text2, d_roff2, d_scan;
  Event ev_up, ev_rec, ev_done, t_rec0, t_rec1;
  bool busy = false;
};

// what the steps of one window share (run_pass)
struct Window {
  int si = 0;               // the slot it goes through
  u64 n = 0, first = 0;     // records (pairs) it takes, and the index of the first
  u64 nb[2] = {0, 0};       // per mate: bytes of names,
  u32 ndir[2] = {0, 0};     // entries of the bucket directory
  u64 slice[2] = {0, 0};    // and bytes of the read stream
  u64 nbytes = 0, cut = 0;  // text that comes down; what the strip takes off it on the device
  bool strip = false;
};

struct Job {
  int slot, mate;
  u64 first, n, nbytes;
  int kind = 0;  // 0: a window for wr; 1: a window for the spill; 2: a stripe for wr (the last two: the order restore)
};

// The order restore (scalce_stream_decompress_restore).  Pass B is the window loop: a window's records are grouped by stripe
// on the device and its text, entries and record sizes appended to the spill by the writer thread.  Pass C reads the spill
// back stripe by stripe, puts the records in their places on the device and hands each stripe to wr.
struct RestoreSlot {
  HBuf h_ord, h_gidx, h_groff, h_counts, h_bad;
  DBuf d_ord, d_sidx, d_gidx, d_gtext, d_groff, d_counts, d_bad, d_ws;
};
struct Restore {
  scalce_restore_params P;
  scalce_restore_stats S;
  Src o;                       // the order stream of the pass that runs
  u64 delivered = 0, skipped = 0;
  u64 N = 0, taken = 0;        // entries its header promises; entries the windows have taken
  u64 R = 0, NS = 0;           // records per stripe, stripes (scalce_order_plan)
  u64 rcap = 0;                // records a buffer of record words holds: a window's or a stripe's, whichever is more
  std::string dir;
  int fd_text = -1, fd_rec = -1;
  scalce_host::StripeTable table;
  std::vector<u64> words;      // a window's / a stripe's record words: entry | size << 32
  RestoreSlot rs[2];
  ~Restore() { if (fd_text >= 0) ::close(fd_text); if (fd_rec >= 0) ::close(fd_rec); }
};

struct Session {
  scalce_ctx *ctx;
  scalce_unpack_params P;
  scalce_write_fn wr;
  void *wr_user;
  scalce_unpack_stats S;
  scalce_unpack_range RG;
  scalce_unpack_range_stats RS;
  Failure F;
  std::atomic<bool> failed{false};
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool closing = false;
  std::thread writer;
  int device = 0;
  std::unique_ptr<Restore> X;  // set: the input order is restored

  // (the streams in front of what is used on them: close() lets everything go in the right order by hand, and should a
  // session ever die without it, the buffers and events would still go before the streams)
  Stream s_up, s_main, s_dec, s_down;
  Mate M[2];
  Slot slot[2];
  int m0 = 0, m1 = 0;  // the mates of the pass that runs (one mate, or both under -i)
  bool known = false;  // ... and whether a symbol count says how many records they hold
  bool names = false, qual = true;
  std::string library;
  u64 W = 0, R = 0, D = 0, cap_in = 0, cap_text = 0;
  u64 live = 0;
  u64 widx = 0;

  Session(scalce_ctx *c, const scalce_unpack_params *p, const scalce_unpack_range *rg, scalce_write_fn w, void *wu)
      : ctx(c), P(*p), wr(w), wr_user(wu) {
    memset(&S, 0, sizeof S);
    S.error_mate = S.error_stream = -1;
    memset(&RG, 0, sizeof RG);
    RG.nrecords = UNKNOWN;
    if (rg) RG = *rg;
    memset(&RS, 0, sizeof RS);
    RS.first_record = RG.first_record;
    RS.total_records = UNKNOWN;
  }

  // ---- errors: the first one stays, nothing further is launched behind it ------------------------------------------------
  int fail(int rc, int mate, int stream, int wants_file, const char *fmt, ...) {
    char b[600];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(mu);
    if (F.rc == SCALCE_OK) { F.rc = rc; F.msg = b; F.mate = mate; F.stream = stream; F.wants_file = wants_file; }
    failed = true;
    cv.notify_all();
    return F.rc;
  }
  int hip(hipError_t e, const char *what) { return e == hipSuccess ? SCALCE_OK : fail(SCALCE_ERR_HIP, -1, -1, 0, "%s: %s", what, hipGetErrorString(e)); }
  int lib(int rc) { return rc ? fail(rc, -1, -1, 0, "%s", scalce_last_error(ctx)) : SCALCE_OK; }
#define SD_HIP(expr) do { if (int rc_ = hip((expr), #expr)) return rc_; } while (0)
#define SD_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

  // a stream that ends, or fails, before what is asked of it (stream: 0 r, 1 n, 2 q, 3 l)
  Src &src(int m, int stream) { return stream == 0 ? M[m].r : stream == 1 ? M[m].n : stream == 2 ? M[m].q : stream == 3 ? M[m].l : X->o; }
  static const char *stream_name(int stream) {
    return stream == 0 ? "read" : stream == 1 ? "name" : stream == 2 ? "quality" : stream == 3 ? "length" : "order";
  }
  int read_error(int m, int stream) { return fail(SCALCE_ERR_FORMAT, m, stream, 0, "read error on the %s stream", stream_name(stream)); }
  int truncated(int m, int stream) { return fail(SCALCE_ERR_FORMAT, m, stream, 0, "(ERROR) truncated %s stream", stream_name(stream)); }
  int short_stream(int m, int stream) { return src(m, stream).bad ? read_error(m, stream) : truncated(m, stream); }

  // device memory is counted where it comes and goes: `live` is the sum of the buffers' cap (and of the decoders' tables)
  int dmalloc(DBuf &b, u64 bytes) {
    SD_HIP(dbuf_alloc(b, bytes));
    live += b.cap;
    S.peak_device_bytes = std::max(S.peak_device_bytes, live);
    return SCALCE_OK;
  }
  void drop(DBuf &b) { live -= b.cap; b.release(); }
  int hmalloc(HBuf &b, u64 bytes) {
    SD_HIP(b.alloc(bytes));
    S.pinned_host_bytes += b.cap;
    return SCALCE_OK;
  }

  // ---- headers (decompress.cpp:131-237) ------------------------------------------------------------------------------
  int headers(scalce_read_fn rd[2][3], void *user[2][3]) {
    qual = !P.no_qualities;
    for (int m = 0; m < P.mates; m++) {
      Mate &x = M[m];
      x.r.open(rd[m][0], RG.skip[m][0], user[m][0], &S.read_wait_s, &RS.bytes_delivered[m][0], &RS.bytes_skipped[m][0]);
      x.n.open(rd[m][1], RG.skip[m][1], user[m][1], &S.read_wait_s, &RS.bytes_delivered[m][1], &RS.bytes_skipped[m][1]);
      x.q.open(qual ? rd[m][2] : nullptr, RG.skip[m][2], qual ? user[m][2] : nullptr, &S.read_wait_s, &RS.bytes_delivered[m][2],
               &RS.bytes_skipped[m][2]);
      if (!x.r.need(8) || memcmp(x.r.ptr(), "scalce2", 7)) return fail(SCALCE_ERR_FORMAT, m, 0, 1, "is not a scalce archive");
      const bool has_no_ac = x.r.ptr()[6] == '2' && x.r.ptr()[7] >= '2';
      x.r.skip(8);
      int32_t v = 0;
      if (has_no_ac) {
        if (!x.r.need(4)) return truncated(m, 0);
        memcpy(&v, x.r.ptr(), 4); x.r.skip(4);
        x.no_ac = v;
      }
      if (!x.r.need(4)) return truncated(m, 0);
      memcpy(&v, x.r.ptr(), 4); x.r.skip(4);
      x.L = v;
      if (x.L <= 0) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) read length %d in the read stream's header", x.L);
      if (x.r.bad) return read_error(m, 0);
      if (qual) {
        if (x.q.need(16)) { memcpy(&x.phred, x.q.ptr() + 8, 8); x.q.skip(16); } else x.q.skip(x.q.avail());
        x.q_empty = !x.q.need(1);
        if (x.q.bad) return read_error(m, 2);
      }
      if (x.n.need(8)) x.n.skip(8);
      if (P.len_rd[m]) {  // the fourth stream: header, then one entry per record
        x.l.open(P.len_rd[m], P.len_skip[m], P.len_user[m], &S.read_wait_s, &x.l_delivered, &x.l_skipped);
        int hl = 0;
        const bool whole = x.l.need(scalce_host::LEN_HEADER_BYTES);
        if (x.l.bad) return read_error(m, 3);
        if (const char *why = scalce_host::len_header_read(x.l.ptr(), whole ? scalce_host::LEN_HEADER_BYTES : 0, &x.l_width, &hl))
          return fail(SCALCE_ERR_FORMAT, m, 3, 0, "(ERROR) %s", why);
        x.l.skip(scalce_host::LEN_HEADER_BYTES);
        if (hl != x.L)
          return fail(SCALCE_ERR_FORMAT, m, 3, 0, "(ERROR) the length stream was written for reads of up to %d bases, the read stream holds reads of %d", hl, x.L);
        x.has_len = true;
      }
    }
    if (P.ignore_names) {
      library = P.library ? P.library : "";
    } else {
      u8 nm = 0;
      for (int m = 0; m < P.mates; m++)
        if (M[m].n.need(1)) { nm = M[m].n.ptr()[0]; M[m].n.skip(1); }
      names = nm != 0;
      if (!names)
        for (int m = 0; m < P.mates; m++) {  // int64 0, then the library name to the end of the stream
          Src &n = M[m].n;
          if (n.need(8)) n.skip(8);
          library.clear();
          while (n.need(1)) { library.append((const char *)n.ptr(), n.avail()); n.skip(n.avail()); if (library.size() > 4096) break; }
        }
    }
    if (!names && library.size() > 255) return fail(SCALCE_ERR_ARG, -1, 1, 0, "library name longer than 255 characters");
    if (P.interleave && M[0].no_ac != M[1].no_ac) return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) the mates were not archived together");
    return SCALCE_OK;
  }

  // ---- mate 1's buckets ----------------------------------------------------------------------------------------------
  // moves to the next bucket that has records; 0: there is one, 1: the stream has ended, < 0: failed
  int next_bucket(int m, size_t look = ~(size_t)0) {
    Mate &x = M[m];
    while (!x.bk.left) {
      if (!x.r.need(12, look)) {
        if (x.r.bad) { read_error(m, 0); return -1; }
        return 1;
      }
      int32_t core;
      u64 cnt;
      memcpy(x.bk.header, x.r.ptr(), 12);
      memcpy(&core, x.r.ptr(), 4);
      memcpy(&cnt, x.r.ptr() + 4, 8);
      x.r.skip(12);
      x.bk.core_len = 0;
      if (core != SCALCE_ROOT_CORE) {
        const int cl = scalce_pattern_length(ctx, core);
        const char *cs = scalce_pattern_string(ctx, core);
        if (core < 0 || core >= scalce_patterns_count(ctx) || cl < 0 || !cs) {
          fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) archive refers to core %d which the core table does not have", core);
          return -1;
        }
        if (cl > (int)sizeof x.bk.core || cl > x.L) { fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) core %d does not fit the reads", core); return -1; }
        x.bk.core_len = (u32)cl;
        memcpy(x.bk.core, cs, (size_t)cl);
      }
      x.bk.rec_bytes = (u32)((x.L - (int)x.bk.core_len + 3) / 4) + (x.L > 255 ? 2u : 1u);
      x.bk.left = cnt;
    }
    return 0;
  }

  // ---- sizes and buffers: from the window, the read lengths and the table, never from the archive --------------------------
  u64 rec_fixed(int m) const { return (qual ? 2ull : 1ull) * (u64)M[m].L + (qual ? 6 : 3); }
  // text of records [first, first + n) of mate m when names are made up: "<library>.<index>"
  u64 lib_text(int m, u64 first, u64 n, bool with_qual) const {
    auto f = with_qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes;
    return f(M[m].L, first + n, 0, library.c_str()) - f(M[m].L, first, 0, library.c_str());
  }
  u64 lib_text(int m, u64 first, u64 n) const { return lib_text(m, first, n, qual); }
  // What a window is measured in: bytes of FASTQ text, four lines per record, whether or not the archive holds qualities.
  // The two-line records of -Q / -f are cut at the same records as their FASTQ would be, so the records per window -- and
  // with them every buffer -- depend on the window and the read length alone.
  u64 rec_budget(int m) const { return 2ull * (u64)M[m].L + 6; }

  int setup_slots() {  // mates m0 .. m1 share a window
    W = P.window_text_bytes ? P.window_text_bytes : SCALCE_WINDOW_TEXT_DEFAULT;
    S.window_text_bytes = W;
    u64 rec_min = 0, rec_max = 0;
    for (int m = m0; m <= m1; m++) { rec_min += rec_budget(m); rec_max += rec_fixed(m) + 255 + 32; }
    R = std::max<u64>(1, W / rec_min);
    D = std::min<u64>(R, (u64)scalce_patterns_count(ctx) + 2);
    cap_text = std::max(W, rec_max) + 64;
    u64 rcap = R;
    if (X) {  // a stripe's text fits the window's bound, unless the cap on the stripes raised R
      u64 pl[2];
      scalce_host::order_plan(X->N, W, rec_max, pl);
      X->R = pl[0]; X->NS = pl[1];
      X->S.stripe_records = pl[0]; X->S.stripes = pl[1];
      X->table.reset(X->NS);
      cap_text = std::max(cap_text, X->R * rec_max + 64);
      rcap = X->rcap = std::max(R, X->R);
    }
    const u64 roff_bytes = 8 * (rcap + 1), len_bytes = 2 * R + 64;
    u64 o = 0;
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      const u64 rb_max = (u64)(x.L + 3) / 4 + 2;
      x.cap_slice = R * rb_max + 12 * D;
      x.o_reads = o; o = align_up(o + x.cap_slice + 64, 256);
      x.o_dir = o; o = align_up(o + sizeof(scalce_fq_bucket) * D, 256);
      if (names) {
        x.cap_names = std::min(cap_text, R * 256);
        x.o_names = o; o = align_up(o + x.cap_names + 64, 256);
        x.o_noff = o; o = align_up(o + roff_bytes, 256);
      }
      if (qual && x.no_ac) { x.o_qual = o; o = align_up(o + R * (u64)x.L + 64, 256); }
    }
    cap_in = o;
    for (int i = 0; i < 2; i++) {
      Slot &s = slot[i];
      SD_TRY(hmalloc(s.h_in, cap_in));
      SD_TRY(dmalloc(s.d_in, cap_in));
      SD_TRY(hmalloc(s.h_text, cap_text));
      SD_TRY(dmalloc(s.d_text, cap_text));
      const bool strip = M[m0].has_len;  // (never with two mates in one window: -d -i refuses a length stream)
      if (P.split) SD_TRY(hmalloc(s.h_roff, roff_bytes));
      if (P.split || strip || X) SD_TRY(dmalloc(s.d_roff, roff_bytes));
      if (X) {
        RestoreSlot &q = X->rs[i];
        const u64 words = 4 * rcap + 64, ws = std::max(scalce_order_group_ws_bytes(rcap, X->NS), scalce_records_permute_ws_bytes(rcap));
        for (HBuf *b : {&q.h_ord, &q.h_gidx}) SD_TRY(hmalloc(*b, words));
        SD_TRY(hmalloc(q.h_groff, roff_bytes));
        SD_TRY(hmalloc(q.h_counts, 4 * X->NS + 64));
        SD_TRY(hmalloc(q.h_bad, 64));
        for (DBuf *b : {&q.d_ord, &q.d_sidx, &q.d_gidx}) SD_TRY(dmalloc(*b, words));
        SD_TRY(dmalloc(q.d_gtext, cap_text));
        SD_TRY(dmalloc(q.d_groff, roff_bytes));
        SD_TRY(dmalloc(q.d_counts, 4 * X->NS + 64));
        SD_TRY(dmalloc(q.d_bad, 64));
        SD_TRY(dmalloc(q.d_ws, ws));
      }
      if (strip) {
        SD_TRY(hmalloc(s.h_len, len_bytes));
        SD_TRY(dmalloc(s.d_len, len_bytes));
        SD_TRY(dmalloc(s.d_text2, cap_text));
        SD_TRY(dmalloc(s.d_roff2, roff_bytes));
        SD_TRY(dmalloc(s.d_scan, scalce_fastq_strip_ws_bytes(R)));
      }
      for (Event *e : {&s.ev_up, &s.ev_rec, &s.ev_done}) SD_HIP(e->create());
      for (Event *e : {&s.t_rec0, &s.t_rec1}) SD_HIP(e->create(true));  // these two are read for the kernels' time
    }
    return SCALCE_OK;
  }
  void free_slots() {
    for (Slot &s : slot) {
      for (DBuf *b : {&s.d_len, &s.d_text2, &s.d_roff2, &s.d_scan, &s.d_in, &s.d_text, &s.d_roff}) drop(*b);
      s = Slot();
    }
    if (X)
      for (RestoreSlot &q : X->rs) {
        for (DBuf *b : {&q.d_ord, &q.d_sidx, &q.d_gidx, &q.d_gtext, &q.d_groff, &q.d_counts, &q.d_bad, &q.d_ws}) drop(*b);
        q = RestoreSlot();
      }
  }

  // the quality stream behind its header: the table, the symbol count, then the frames -- and the decoder for them
  int setup_decoder(int m) {
    Mate &x = M[m];
    Decoder &d = x.d;
    if (!qual || x.no_ac || x.q_empty) return SCALCE_OK;
    std::vector<u32> table(TABLE_BYTES / 4);
    if (x.q.read_into(reinterpret_cast<u8 *>(table.data()), TABLE_BYTES) != TABLE_BYTES) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality table");
    if (!x.q.need(8)) return truncated(m, 2);
    memcpy(&x.total_syms, x.q.ptr(), 8);
    x.q.skip(8);
    x.records_left = x.total_syms / (u64)x.L;
    x.syms_left = x.total_syms;
    x.frames_left = (x.total_syms + FRAME - 1) / FRAME;
    scalce_ac_decoder *dec = nullptr;
    SD_TRY(lib(scalce_ac_decoder_create(ctx, table.data(), s_dec, &dec)));
    d.dec.reset(dec);
    live += scalce_ac_decoder_device_bytes(dec);
    S.peak_device_bytes = std::max(S.peak_device_bytes, live);
    d.G = std::max<u64>(1, (SCALCE_DECODE_AHEAD * R * (u64)x.L + FRAME - 1) / FRAME);
    d.ycap = (u64)x.L + d.G * FRAME + 256;
    // a frame of quality strings codes to a third of its symbols; a batch whose frames do not fit the staging is cut short
    // (at least one frame: a single frame larger than this is not an archive of this coder)
    d.coded_cap = std::max<u64>(d.G * FRAME / 2, FRAME * 2) + 4096;
    SD_TRY(hmalloc(d.h_coded, d.coded_cap));
    SD_TRY(hmalloc(d.h_bad, 2 * sizeof(u32)));
    SD_HIP(d.ev_coded_up.create());
    for (int i = 0; i < 2; i++) {
      SD_TRY(dmalloc(d.Y[i], d.ycap));
      SD_TRY(dmalloc(d.d_coded[i], d.coded_cap));
      SD_TRY(dmalloc(d.d_off[i], 8 * d.G));
      SD_TRY(dmalloc(d.d_size[i], 4 * (d.G + 1)));
      for (Event *e : {&d.ev_dec[i], &d.ev_rec[i]}) SD_HIP(e->create());
      for (Event *e : {&d.t_dec0[i], &d.t_dec1[i]}) SD_HIP(e->create(true));  // (read for the decoder's time)
    }
    return SCALCE_OK;
  }
  void free_decoder(int m) {
    Decoder &d = M[m].d;
    if (d.dec) live -= scalce_ac_decoder_device_bytes(d.dec.get());
    for (int i = 0; i < 2; i++)
      for (DBuf *b : {&d.Y[i], &d.d_coded[i], &d.d_off[i], &d.d_size[i]}) drop(*b);
    d = Decoder();
  }

  // ---- the decoder's batches ---------------------------------------------------------------------------------------------
  // Batch b = the next whole frames of mate m, up to G of them, decoded into Y[b & 1] behind what batch b - 1 leaves over:
  // windows take whole records, so that carry is have(b - 1) mod L bytes, known before batch b - 1 has been decoded.  Called
  // when the windows of batch b - 2 have all been enqueued: their last records kernel is what the buffer waits for.
  int enqueue_batch(int m) {
    Mate &x = M[m];
    Decoder &d = x.d;
    if (!x.frames_left) return SCALCE_OK;
    const int64_t b = d.enq + 1;
    const int par = (int)(b & 1);
    if (d.coded_up_once) SD_HIP(hipEventSynchronize(d.ev_coded_up));  // the staging's previous bytes have gone up
    u8 *h_coded = d.h_coded.as<u8>(), *Y = d.Y[par].as<u8>();
    u32 *d_size = d.d_size[par].as<u32>();
    u64 at = 0;
    u32 k = 0;
    while (k < d.G && k < x.frames_left) {
      if (!x.q.need(4)) return truncated(m, 2);
      u32 sz;
      memcpy(&sz, x.q.ptr(), 4);
      if (at + 4 + (u64)sz > d.coded_cap - 64) {
        if (k) break;
        return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) a coded block of %u bytes: not a quality stream of this coder", sz);
      }
      memcpy(h_coded + at, &sz, 4);
      x.q.skip(4);
      if (x.q.read_into(h_coded + at + 4, sz) != sz) return truncated(m, 2);
      at += 4 + (u64)sz;
      k++;
    }
    if (x.q.bad) return read_error(m, 2);
    const u64 nsym = std::min<u64>((u64)k * FRAME, x.syms_left);
    // (the first batch of a range begins with x.drop symbols of the records in front of it: they are left where they are
    // decoded and the windows begin behind them, so the carry counts from there)
    const u64 carry = b ? (d.have_b[par ^ 1] - (b == 1 ? x.drop : 0)) % (u64)x.L : 0;
    if (d.rec_once[par]) SD_HIP(hipStreamWaitEvent(s_dec, d.ev_rec[par], 0));
    SD_HIP(hipMemcpyAsync(d.d_coded[par].p, h_coded, at, hipMemcpyHostToDevice, s_dec));
    SD_HIP(hipEventRecord(d.ev_coded_up, s_dec));
    d.coded_up_once = true;
    if (carry) SD_HIP(hipMemcpyAsync(Y, d.Y[par ^ 1].as<u8>() + d.have_b[par ^ 1] - carry, carry, hipMemcpyDeviceToDevice, s_dec));
    SD_HIP(hipEventRecord(d.t_dec0[par], s_dec));
    SD_TRY(lib(scalce_ac_decoder_launch(d.dec.get(), d.d_coded[par].as<u8>(), at, k, nsym, d.d_off[par].as<u64>(), d_size, d_size + d.G, Y + carry, s_dec)));
    SD_HIP(hipEventRecord(d.t_dec1[par], s_dec));
    SD_HIP(hipMemcpyAsync(d.h_bad.as<u32>() + par, d_size + d.G, sizeof(u32), hipMemcpyDeviceToHost, s_dec));
    SD_HIP(hipEventRecord(d.ev_dec[par], s_dec));
    d.have_b[par] = carry + nsym;
    x.frames_left -= k;
    x.syms_left -= nsym;
    d.enq = b;
    S.decode_batches[m]++;
    RS.frames_decoded[m] += k;
    RS.symbols_decoded[m] += nsym;
    return SCALCE_OK;
  }
  // whole records of mate m that the decoded symbols still hold; moves on to the next batch when that is none
  int records_decoded(int m, u64 &n) {
    Mate &x = M[m];
    Decoder &d = x.d;
    const u64 L = (u64)x.L;
    for (;;) {  // (a range's first batch may hold less than one record behind the symbols it drops: then the next one)
      if (d.cur >= 0 && (d.have_b[d.cur & 1] - d.pos) / L) { n = (d.have_b[d.cur & 1] - d.pos) / L; return SCALCE_OK; }
      if (d.cur == d.enq && !x.frames_left) { n = 0; return SCALCE_OK; }
      if (d.enq == d.cur) SD_TRY(enqueue_batch(m));
      d.cur++;
      d.pos = d.cur ? 0 : x.drop;
      SD_TRY(enqueue_batch(m));  // the batch behind it: decoded while this one's windows go through
      const int par = (int)(d.cur & 1);
      SD_HIP(hipEventSynchronize(d.ev_dec[par]));
      float ms = 0;
      SD_HIP(hipEventElapsedTime(&ms, d.t_dec0[par], d.t_dec1[par]));
      S.decode_s += 1e-3 * ms;
      if (d.h_bad.as<u32>()[par]) return truncated(m, 2);
    }
  }

  // ---- the writer: one thread, windows in order ----------------------------------------------------------------------------
  void writer_main() {
    (void)hipSetDevice(device);
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !jobs.empty() || closing; });
        if (jobs.empty()) return;
        j = jobs.front();
        jobs.pop_front();
      }
      Slot &s = slot[j.slot];
      if (!failed) {
        const double t0 = now_s();
        const hipError_t e = hipEventSynchronize(s.ev_done);
        if (e != hipSuccess) hip(e, "a window's text did not come down");
        if (j.kind == 2) X->S.place_wait_s += now_s() - t0;
      }
      if (!failed && j.kind && X->rs[j.slot].h_bad.as<u32>()[0])
        fail(SCALCE_ERR_FORMAT, m0, 4, 0, "(ERROR) %s", scalce_host::order_not_permutation());
      if (!failed && j.kind == 1) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.t_rec0, s.t_rec1) == hipSuccess) S.records_s += 1e-3 * ms;
        spill_window(j);
        S.windows++;
      } else if (!failed) {
        float ms = 0;
        if (!j.kind && hipEventElapsedTime(&ms, s.t_rec0, s.t_rec1) == hipSuccess) S.records_s += 1e-3 * ms;
        const double t0 = now_s();
        if (wr(wr_user, j.mate, j.first, j.n, s.h_text.as<u8>(), j.nbytes, P.split ? s.h_roff.as<u64>() : nullptr)) fail(SCALCE_ERR_FORMAT, j.mate, -1, 0, "the write callback failed");
        S.write_s += now_s() - t0;
        if (!j.kind) S.windows++;
      }
      { std::lock_guard<std::mutex> lk(mu); s.busy = false; }
      cv.notify_all();
    }
  }
  bool wait_slot(int i) {  // false: the session has failed
    const double t0 = now_s();
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !slot[i].busy || failed.load(); });
    S.write_wait_s += now_s() - t0;
    return !failed;
  }
  void drain() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return (!slot[0].busy && !slot[1].busy) || failed.load(); });
  }

  // ---- the order restore --------------------------------------------------------------------------------------------------
  int order_count(u64 records) {
    char b[200];
    scalce_host::order_count_message(b, sizeof b, X->N, records);
    return fail(SCALCE_ERR_FORMAT, m0, 4, 0, "(ERROR) %s", b);
  }
  int spill_error(const char *what) {
    return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) cannot %s a spill file in %s: %s", what, X->dir.c_str(), strerror(errno));
  }
  // a mate pass begins: the order stream from its start, its header, empty spill files
  int restore_open(int m) {
    Restore &x = *X;
    x.o = Src();
    x.o.open(x.P.order_rd[m], nullptr, x.P.order_user[m], &S.read_wait_s, &x.delivered, &x.skipped);
    const bool whole = x.o.need(scalce_host::ORDER_HEADER_BYTES);
    if (x.o.bad) return read_error(m, 4);
    if (const char *why = scalce_host::order_header_read(x.o.ptr(), whole ? scalce_host::ORDER_HEADER_BYTES : 0, &x.N))
      return fail(SCALCE_ERR_FORMAT, m, 4, 0, "(ERROR) %s", why);
    x.o.skip(scalce_host::ORDER_HEADER_BYTES);
    x.taken = 0;
    for (int *fd : {&x.fd_text, &x.fd_rec}) {
      if (*fd < 0) {  // made once, unlinked at once: nothing stays behind whatever happens
        std::string path = x.dir + "/scalce_order_XXXXXX";
        *fd = mkstemp(&path[0]);
        if (*fd < 0) return spill_error("make");
        unlink(path.c_str());
      } else if (ftruncate(*fd, 0) != 0) return spill_error("empty");
    }
    return SCALCE_OK;
  }
  bool spill_write(int fd, const void *p, u64 n, u64 at) {
    const u8 *b = static_cast<const u8 *>(p);
    const double t0 = now_s();
    while (n) {
      const ssize_t k = ::pwrite(fd, b, (size_t)std::min<u64>(n, 1u << 30), (off_t)at);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) { if (!k) errno = ENOSPC; X->S.spill_write_s += now_s() - t0; return false; }
      b += k; n -= (u64)k; at += (u64)k;
    }
    X->S.spill_write_s += now_s() - t0;
    return true;
  }
  bool spill_read(int fd, void *p, u64 n, u64 at) {
    u8 *b = static_cast<u8 *>(p);
    const double t0 = now_s();
    while (n) {
      const ssize_t k = ::pread(fd, b, (size_t)std::min<u64>(n, 1u << 30), (off_t)at);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) { if (!k) errno = EIO; X->S.spill_read_s += now_s() - t0; return false; }
      b += k; n -= (u64)k; at += (u64)k;
    }
    X->S.spill_read_s += now_s() - t0;
    return true;
  }
  // (the writer thread) a window's grouped records behind the spill's end; the table learns where its shares lie
  void spill_window(const Job &j) {
    Restore &x = *X;
    const RestoreSlot &q = x.rs[j.slot];
    const u64 *off = q.h_groff.as<u64>();
    const u32 *idx = q.h_gidx.as<u32>();
    const u64 text_at = x.table.text_bytes, rec_at = x.table.records;
    if (off[j.n] - off[0] != j.nbytes || !x.table.add_window(q.h_counts.as<u32>(), off, j.n)) {
      fail(SCALCE_ERR_FORMAT, m0, 4, 0, "internal: a window's stripes do not add up");
      return;
    }
    x.words.resize(j.n);
    for (u64 k = 0; k < j.n; k++) x.words[k] = (u64)idx[k] | ((off[k + 1] - off[k]) << 32);
    if (!spill_write(x.fd_text, slot[j.slot].h_text.p, j.nbytes, text_at) || !spill_write(x.fd_rec, x.words.data(), 8 * j.n, 8 * rec_at)) {
      spill_error("write");
      return;
    }
    x.S.spilled_bytes += j.nbytes + 8 * j.n;
  }
  // Pass C: stripe s holds the records of input index [s R, s R + expect).  Every window's share comes back from the spill,
  // goes up, the records find their places and the stripe goes to wr through the writer thread, slot by slot in turn.
  int restore_stripes() {
    Restore &x = *X;
    const int mate = m1 > m0 ? 0 : m0;
    std::vector<scalce_host::StripeTable::Piece> pieces;
    for (u64 s = 0; s < x.NS; s++) {
      if (failed) return F.rc;
      const u64 base = s * x.R, expect = std::min(x.R, x.N - base);
      u64 bytes = 0;
      const u64 m = x.table.take_stripe(pieces, &bytes);
      if (m != expect) return fail(SCALCE_ERR_FORMAT, m0, 4, 0, "(ERROR) %s", scalce_host::order_not_permutation());
      if (bytes + 64 > cap_text || m > x.rcap) return fail(SCALCE_ERR_CAPACITY, -1, -1, 0, "internal: a stripe of %llu bytes of text", (unsigned long long)bytes);
      const int si = (int)(s & 1);
      if (!wait_slot(si)) return F.rc;
      Slot &sl = slot[si];
      RestoreSlot &q = x.rs[si];
      x.words.resize(m);
      u64 tb = 0, tr = 0;
      for (const auto &pc : pieces) {
        if (!spill_read(x.fd_text, sl.h_text.as<u8>() + tb, pc.bytes, pc.text_at) || !spill_read(x.fd_rec, x.words.data() + tr, 8 * pc.records, 8 * pc.record_at))
          return spill_error("read");
        tb += pc.bytes; tr += pc.records;
      }
      u64 *off = q.h_groff.as<u64>();
      u32 *idx = q.h_ord.as<u32>();
      off[0] = 0;
      for (u64 k = 0; k < m; k++) { idx[k] = (u32)x.words[k]; off[k + 1] = off[k] + (x.words[k] >> 32); }
      if (off[m] != bytes) return fail(SCALCE_ERR_FORMAT, m0, 4, 0, "internal: a stripe's record sizes do not add up");
      SD_HIP(hipMemcpyAsync(sl.d_text.p, sl.h_text.p, bytes, hipMemcpyHostToDevice, s_main));
      SD_HIP(hipMemcpyAsync(sl.d_roff.p, off, 8 * (m + 1), hipMemcpyHostToDevice, s_main));
      SD_HIP(hipMemcpyAsync(q.d_ord.p, idx, 4 * m, hipMemcpyHostToDevice, s_main));
      SD_TRY(lib(scalce_order_place(ctx, q.d_ord.as<u32>(), m, base, expect, q.d_sidx.as<u32>(), q.d_bad.as<u32>(), s_main)));
      SD_TRY(lib(scalce_records_permute(ctx, sl.d_text.as<u8>(), sl.d_roff.as<u64>(), m, bytes, q.d_sidx.as<u32>(), q.d_gtext.as<u8>(), cap_text,
                                        q.d_groff.as<u64>(), q.d_ws.p, s_main)));
      SD_HIP(hipMemcpyAsync(sl.h_text.p, q.d_gtext.p, bytes, hipMemcpyDeviceToHost, s_main));
      if (P.split) SD_HIP(hipMemcpyAsync(sl.h_roff.p, q.d_groff.p, 8 * (m + 1), hipMemcpyDeviceToHost, s_main));
      SD_HIP(hipMemcpyAsync(q.h_bad.p, q.d_bad.p, 4, hipMemcpyDeviceToHost, s_main));
      SD_HIP(hipEventRecord(sl.ev_done, s_main));
      {
        std::lock_guard<std::mutex> lk(mu);
        sl.busy = true;
        jobs.push_back(Job{si, mate, base, expect, bytes, 2});
      }
      cv.notify_all();
    }
    drain();
    x.S.records = x.N;
    return failed ? F.rc : SCALCE_OK;
  }

  // ---- which stream says how many records there are ---------------------------------------------------------------------
  // Where no symbol count says how many records the archive holds (`known`), the streams that end it for a whole run -- the
  // names, else the raw quality rows, else the read stream, of the pass's first mate -- end it in front of a range too: a
  // range that begins behind them is empty.  A short read on the stream that decides (0 r, 1 n, 2 q) ends the archive and is
  // no error; any other stream that ends in front of the range, or inside a window, is truncated.
  bool decides_count(int m, int stream) const {
    if (known || m != m0) return false;
    return stream == 1 || (!names && (stream == 2 || !(qual && M[m].no_ac)));
  }
  // does mate m's read stream hold another record (mate 2, which has no headers: another `least` bytes)?
  int more_reads(int m, size_t least, bool &more) {
    if (m != 0) { more = M[m].r.need(least); return SCALCE_OK; }
    const int e = next_bucket(0);
    more = e == 0;
    return e < 0 ? F.rc : SCALCE_OK;
  }

  // ---- one window --------------------------------------------------------------------------------------------------------
  // names of up to `ncap` records (pairs) into the slot, as many as the window's text takes; n = how many
  int take_names(Slot &s, u64 ncap, u64 &n, u64 nb[2]) {
    u64 text = 0;
    nb[0] = nb[1] = 0;
    n = 0;
    u8 *h_in = s.h_in.as<u8>();
    u64 *noff[2] = {reinterpret_cast<u64 *>(h_in + M[m0].o_noff), reinterpret_cast<u64 *>(h_in + M[m1].o_noff)};
    u8 *dst[2] = {h_in + M[m0].o_names, h_in + M[m1].o_names};
    const int nmates = m1 - m0 + 1;
    while (n < ncap) {
      u32 len[2] = {0, 0};
      int ended = 0;
      u64 rec = 0;
      for (int i = 0; i < nmates; i++) {
        Src &src = M[m0 + i].n;
        if (!src.need(1)) { ended++; continue; }
        len[i] = src.ptr()[0];
        if (!src.need(1 + (size_t)len[i])) return truncated(m0 + i, 1);
        rec += len[i] + rec_budget(m0 + i);
      }
      if (ended) {
        for (int i = 0; i < nmates; i++) if (M[m0 + i].n.bad) return read_error(m0 + i, 1);
        if (!decides_count(m0, 1) || ended != nmates) return truncated(m0, 1);
        break;
      }
      if (n && text + rec > W) break;
      bool fits = true;
      for (int i = 0; i < nmates; i++) fits = fits && nb[i] + 1 + len[i] <= M[m0 + i].cap_names;
      if (!fits) break;
      for (int i = 0; i < nmates; i++) {
        Src &src = M[m0 + i].n;
        noff[i][n] = nb[i];
        memcpy(dst[i] + nb[i], src.ptr(), 1 + (size_t)len[i]);
        src.skip(1 + (size_t)len[i]);
        nb[i] += 1 + len[i];
      }
      text += rec;
      n++;
    }
    for (int i = 0; i < nmates; i++) noff[i][n] = nb[i];
    return SCALCE_OK;
  }
  // n records of mate m's read stream into the slot; got < n: the stream has ended
  int take_reads(Slot &s, int m, u64 n, u64 &got, u32 &ndir, u64 &slice) {
    Mate &x = M[m];
    u8 *dst = s.h_in.as<u8>() + x.o_reads;
    scalce_fq_bucket *dir = reinterpret_cast<scalce_fq_bucket *>(s.h_in.as<u8>() + x.o_dir);
    got = 0; ndir = 0; slice = 0;
    if (m != 0) {  // bare records in mate 1's order
      const u64 rb = (u64)(x.L + 3) / 4;
      const u64 bytes = x.r.read_into(dst, n * rb);
      if (x.r.bad) return read_error(m, 0);
      got = bytes / rb;
      if (bytes % rb) return truncated(m, 0);
      memset(&dir[0], 0, sizeof dir[0]);
      dir[0].rec_bytes = (u32)rb;
      ndir = 1; slice = bytes;
      return SCALCE_OK;
    }
    while (got < n) {
      if (!x.bk.left) {
        const int e = next_bucket(m);
        if (e < 0) return F.rc;
        if (e) break;
        if (got) { memcpy(dst + slice, x.bk.header, 12); slice += 12; }  // headers inside the slice stay inline
      }
      if (ndir == D) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) the read stream opens more buckets than the core table has cores");
      const u64 t = std::min(x.bk.left, n - got), bytes = t * x.bk.rec_bytes;
      if (slice + bytes > x.cap_slice) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) the read stream opens more buckets than the core table has cores");
      if (x.r.read_into(dst + slice, bytes) != bytes) return short_stream(m, 0);
      scalce_fq_bucket &b = dir[ndir++];
      memset(&b, 0, sizeof b);
      b.first = got; b.off = slice; b.core_len = x.bk.core_len; b.rec_bytes = x.bk.rec_bytes;
      memcpy(b.core, x.bk.core, x.bk.core_len);
      slice += bytes; got += t; x.bk.left -= t;
    }
    return SCALCE_OK;
  }

  // ---- the range: what lies in front of its first record is passed over, stream by stream -------------------------------
  // Nothing of it reaches the device.  A stream that decides the record count (decides_count) may end in front of the range,
  // which is empty then.
  int pass_over() {
    u64 first = RG.first_record;
    if (known) { RS.total_records = M[m0].records_left; first = std::min(first, M[m0].records_left); }
    constexpr size_t LOOK = 64u << 10;  // read ahead of a bucket header when the bucket behind it is skipped, not read
    if (names)  // a length byte per name has to be read: the names go through the look-ahead buffer, not through skip
      for (int m = m0; m <= m1; m++) {
        Src &src = M[m].n;
        u64 k = 0;
        for (; k < first && src.need(1); k++) {
          const size_t len = src.ptr()[0];
          if (!src.need(1 + len)) return short_stream(m, 1);
          src.skip(1 + len);
        }
        if (src.bad) return read_error(m, 1);
        if (k < first) {
          if (!decides_count(m, 1)) return truncated(m, 1);
          first = k;
        }
      }
    for (int m = m0; m <= m1; m++) {  // -A: rows of L bytes
      Mate &x = M[m];
      if (!qual || !x.no_ac) continue;
      const u64 want = first * (u64)x.L, bytes = x.q.pass(want);
      if (x.q.bad) return read_error(m, 2);
      if (bytes != want) {
        if (!decides_count(m, 2) || bytes % (u64)x.L) return truncated(m, 2);
        first = bytes / (u64)x.L;
      }
    }
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      u64 got = 0;
      if (m != 0) {
        const u64 rb = (u64)(x.L + 3) / 4, bytes = x.r.pass(first * rb);
        if (bytes % rb && !x.r.bad) return truncated(m, 0);
        got = bytes / rb;
      } else {
        while (got < first) {  // bucket by bucket: every header is read and checked, the records behind it are not
          if (!x.bk.left) {
            const int e = next_bucket(m, x.r.skp ? LOOK : ~(size_t)0);
            if (e < 0) return F.rc;
            if (e) break;
          }
          const u64 t = std::min(x.bk.left, first - got), bytes = t * x.bk.rec_bytes;
          if (x.r.pass(bytes) != bytes) return short_stream(m, 0);
          got += t; x.bk.left -= t;
        }
      }
      if (x.r.bad) return read_error(m, 0);
      if (got != first) {
        if (!decides_count(m, 0)) return truncated(m, 0);
        first = got;
      }
    }
    for (int m = m0; m <= m1; m++) {  // coded qualities: whole frames by their size words, then the symbols in front of the record
      Mate &x = M[m];
      if (!x.d.dec) continue;
      u64 pl[4];
      if (scalce_range_plan_quality(x.L, first, RG.nrecords, x.total_syms, pl)) return fail(SCALCE_ERR_ARG, m, 2, 0, "internal: the range's plan");
      for (u64 f = 0; f < pl[0]; f++) {
        if (!x.q.need(4, x.q.skp ? 0 : ~(size_t)0)) return short_stream(m, 2);
        u32 sz;
        memcpy(&sz, x.q.ptr(), 4);
        x.q.skip(4);
        if (x.q.pass(sz) != sz) return short_stream(m, 2);
      }
      RS.frames_passed[m] = pl[0];
      x.frames_left = pl[1];
      x.drop = pl[2];
      x.syms_left = pl[2] + pl[3];
    }
    for (int m = m0; m <= m1; m++) {  // the length stream: entries of one width
      Mate &x = M[m];
      if (!x.has_len) continue;
      const u64 want = first * (u64)x.l_width;
      if (x.l.pass(want) != want) return short_stream(m, 3);
    }
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      x.first = first;
      x.range_left = RG.nrecords;
      if (known) x.records_left -= first;
    }
    RS.first_record = first;
    return SCALCE_OK;
  }

  // ---- the steps of a window, in the order run_pass() takes them ---------------------------------------------------------
  // How many records: what the decoders hold, what the range and the archive leave, then what the text takes -- with names
  // they come into the slot as they are counted, made-up names are bisected.  w.n stays 0: nothing is left
  int window_records(Window &w) {
    u64 ncap = std::min(R, std::min(M[m0].records_left, M[m0].range_left));
    for (int m = m0; m <= m1 && ncap; m++)
      if (M[m].d.dec) { u64 k; SD_TRY(records_decoded(m, k)); ncap = std::min(ncap, k); }
    if (X) ncap = std::min(ncap, X->N - X->taken);  // (records behind the last entry: check_end reports them)
    if (!ncap) return SCALCE_OK;
    w.si = (int)(widx & 1);
    if (!wait_slot(w.si)) return F.rc;
    w.n = ncap;
    w.first = M[m0].first;
    if (names) return take_names(slot[w.si], ncap, w.n, w.nb);
    auto text = [&](u64 k) { u64 t = 0; for (int m = m0; m <= m1; m++) t += lib_text(m, w.first, k, true); return t; };
    if (text(w.n) > W) {
      u64 lo = 1, hi = w.n;  // text(lo) fits (or lo = 1), text(hi) does not
      while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (text(mid) <= W) lo = mid; else hi = mid; }
      w.n = lo;
    }
    return SCALCE_OK;
  }
  // The pinned block from the other streams: raw quality rows, reads, length entries.  A stream that decides the record
  // count may make the window shorter (w.n == 0: the archive ends here); then the text's size is known
  int window_fill(Window &w) {
    Slot &s = slot[w.si];
    for (int m = m0; m <= m1 && w.n; m++) {  // -A: the q - offset rows as they are
      Mate &x = M[m];
      if (!qual || !x.no_ac) continue;
      const u64 bytes = x.q.read_into(s.h_in.as<u8>() + x.o_qual, w.n * (u64)x.L);
      if (x.q.bad) return read_error(m, 2);
      if (bytes != w.n * (u64)x.L) {
        if (!decides_count(m, 2) || bytes % (u64)x.L) return truncated(m, 2);
        w.n = bytes / (u64)x.L;
      }
    }
    for (int m = m0; m <= m1 && w.n; m++) {
      u64 got = 0;
      SD_TRY(take_reads(s, m, w.n, got, w.ndir[m - m0], w.slice[m - m0]));
      if (got != w.n) {
        if (!decides_count(m, 0)) return truncated(m, 0);
        w.n = got;
      }
    }
    if (!w.n) return SCALCE_OK;
    // variable-length: the window's entries; their sum says how much shorter the text comes down than it is made
    w.strip = M[m0].has_len;
    if (w.strip) {
      Mate &x = M[m0];
      const u64 want = w.n * (u64)x.l_width;
      if (x.l.read_into(s.h_len.as<u8>(), want) != want) return short_stream(m0, 3);
      const u64 sum = scalce_host::len_entries_sum(s.h_len.as<u8>(), w.n, x.l_width, x.L);
      if (sum == ~0ull) return fail(SCALCE_ERR_FORMAT, m0, 3, 0, "(ERROR) the length stream holds an entry above the read length %d", x.L);
      w.cut = 2 * sum;
    }
    if (X) {  // the window's entries of the order stream
      const u64 want = 4 * w.n;
      if (X->o.read_into(X->rs[w.si].h_ord.as<u8>(), want) != want) return short_stream(m0, 4);
      X->taken += w.n;
    }
    for (int m = m0; m <= m1; m++)
      w.nbytes += names ? (qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes)(M[m].L, w.n, w.nb[m - m0], nullptr) : lib_text(m, w.first, w.n);
    if (w.nbytes + 64 > cap_text) return fail(SCALCE_ERR_CAPACITY, -1, -1, 0, "internal: a window of %llu bytes of text", (unsigned long long)w.nbytes);
    return SCALCE_OK;
  }
  int window_upload(const Window &w) {
    Slot &s = slot[w.si];
    u8 *h_in = s.h_in.as<u8>(), *d_in = s.d_in.as<u8>();
    if (w.strip) SD_HIP(hipMemcpyAsync(s.d_len.p, s.h_len.p, w.n * (u64)M[m0].l_width, hipMemcpyHostToDevice, s_up));
    if (X) SD_HIP(hipMemcpyAsync(X->rs[w.si].d_ord.p, X->rs[w.si].h_ord.p, 4 * w.n, hipMemcpyHostToDevice, s_up));
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      const int i = m - m0;
      SD_HIP(hipMemcpyAsync(d_in + x.o_reads, h_in + x.o_reads, w.slice[i], hipMemcpyHostToDevice, s_up));
      SD_HIP(hipMemcpyAsync(d_in + x.o_dir, h_in + x.o_dir, sizeof(scalce_fq_bucket) * w.ndir[i], hipMemcpyHostToDevice, s_up));
      if (names) {
        SD_HIP(hipMemcpyAsync(d_in + x.o_names, h_in + x.o_names, w.nb[i], hipMemcpyHostToDevice, s_up));
        SD_HIP(hipMemcpyAsync(d_in + x.o_noff, h_in + x.o_noff, 8 * (w.n + 1), hipMemcpyHostToDevice, s_up));
      }
      if (qual && x.no_ac) SD_HIP(hipMemcpyAsync(d_in + x.o_qual, h_in + x.o_qual, w.n * (u64)x.L, hipMemcpyHostToDevice, s_up));
    }
    SD_HIP(hipEventRecord(s.ev_up, s_up));
    return SCALCE_OK;
  }
  // records -> text, mate by mate, behind the upload; then the pad goes (variable-length)
  int window_launch(Window &w) {
    Slot &s = slot[w.si];
    u8 *d_in = s.d_in.as<u8>();
    const int nmates = m1 - m0 + 1;
    SD_HIP(hipStreamWaitEvent(s_main, s.ev_up, 0));
    SD_HIP(hipEventRecord(s.t_rec0, s_main));
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      Decoder &d = x.d;
      scalce_fq_window fw;
      memset(&fw, 0, sizeof fw);
      fw.d_reads = d_in + x.o_reads;
      fw.d_dir = reinterpret_cast<const scalce_fq_bucket *>(d_in + x.o_dir);
      fw.nbuckets = w.ndir[m - m0];
      fw.read_len = x.L; fw.has_buckets = m == 0; fw.mate_digit = P.mate_digit ? '1' + m : 0;
      fw.nrecords = w.n; fw.first_record = w.first;
      if (qual) fw.d_qual = x.no_ac ? d_in + x.o_qual : d.Y[d.cur & 1].as<u8>() + d.pos;
      fw.phred_offset = x.phred;
      if (names) { fw.d_names = d_in + x.o_names; fw.d_name_off = reinterpret_cast<const u64 *>(d_in + x.o_noff); }
      fw.library = library.c_str();
      fw.d_out = s.d_text.as<u8>();
      fw.d_record_offsets = ((P.split || w.strip || X) && m == m0) ? s.d_roff.as<u64>() : nullptr;
      if (nmates == 2) {
        const Mate &y = M[m == m0 ? m1 : m0];
        fw.interleave = m - m0 + 1; fw.pair_read_len = y.L;
        if (names) fw.d_pair_name_off = reinterpret_cast<const u64 *>(d_in + y.o_noff);
      }
      SD_TRY(lib(scalce_fastq_records_window(ctx, &fw, s_main)));
      if (d.dec) {
        SD_HIP(hipEventRecord(d.ev_rec[d.cur & 1], s_main));
        d.rec_once[d.cur & 1] = true;
        d.pos += w.n * (u64)x.L;
      }
    }
    if (w.strip) {  // the text and its record offsets come down from the stripped copy
      SD_TRY(lib(scalce_fastq_strip_window(ctx, M[m0].L, w.n, s.d_text.as<u8>(), s.d_roff.as<u64>(), s.d_len.as<u8>(), M[m0].l_width,
                                           s.d_text2.as<u8>(), s.d_roff2.as<u64>(), s.d_scan.p, s_main)));
      w.nbytes -= w.cut;
    }
    if (X) {  // the window's records grouped by the stripe of the output they belong to, and their entries with them
      RestoreSlot &q = X->rs[w.si];
      SD_TRY(lib(scalce_order_group(ctx, q.d_ord.as<u32>(), w.n, X->R, X->N, X->NS, q.d_sidx.as<u32>(), q.d_counts.as<u32>(), q.d_bad.as<u32>(),
                                    q.d_ws.p, s_main)));
      SD_TRY(lib(scalce_records_permute(ctx, (w.strip ? s.d_text2 : s.d_text).as<u8>(), (w.strip ? s.d_roff2 : s.d_roff).as<u64>(), w.n, w.nbytes,
                                        q.d_sidx.as<u32>(), q.d_gtext.as<u8>(), cap_text, q.d_groff.as<u64>(), q.d_ws.p, s_main)));
      SD_TRY(lib(scalce_order_gather(ctx, q.d_ord.as<u32>(), q.d_sidx.as<u32>(), w.n, q.d_gidx.as<u32>(), s_main)));
    }
    SD_HIP(hipEventRecord(s.t_rec1, s_main));
    SD_HIP(hipEventRecord(s.ev_rec, s_main));
    return SCALCE_OK;
  }
  // the text comes down behind the kernels; the writer gets the window
  int window_download(const Window &w) {
    Slot &s = slot[w.si];
    SD_HIP(hipStreamWaitEvent(s_down, s.ev_rec, 0));
    if (X) {  // the grouped text, where its records begin, their entries, the stripes' counts and the verdict
      RestoreSlot &q = X->rs[w.si];
      SD_HIP(hipMemcpyAsync(s.h_text.p, q.d_gtext.p, w.nbytes, hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipMemcpyAsync(q.h_groff.p, q.d_groff.p, 8 * (w.n + 1), hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipMemcpyAsync(q.h_gidx.p, q.d_gidx.p, 4 * w.n, hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipMemcpyAsync(q.h_counts.p, q.d_counts.p, 4 * X->NS, hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipMemcpyAsync(q.h_bad.p, q.d_bad.p, 4, hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipEventRecord(s.ev_done, s_down));
      {
        std::lock_guard<std::mutex> lk(mu);
        s.busy = true;
        jobs.push_back(Job{w.si, m1 > m0 ? 0 : m0, w.first, w.n, w.nbytes, 1});
      }
      cv.notify_all();
      return SCALCE_OK;
    }
    SD_HIP(hipMemcpyAsync(s.h_text.p, w.strip ? s.d_text2.p : s.d_text.p, w.nbytes, hipMemcpyDeviceToHost, s_down));
    if (P.split) SD_HIP(hipMemcpyAsync(s.h_roff.p, w.strip ? s.d_roff2.p : s.d_roff.p, 8 * (w.n + 1), hipMemcpyDeviceToHost, s_down));
    SD_HIP(hipEventRecord(s.ev_done, s_down));
    {
      std::lock_guard<std::mutex> lk(mu);
      s.busy = true;
      jobs.push_back(Job{w.si, m1 > m0 ? 0 : m0, w.first, w.n, w.nbytes, 0});
    }
    cv.notify_all();
    return SCALCE_OK;
  }
  void window_advance(const Window &w) {
    widx++;
    for (int m = m0; m <= m1; m++) {
      M[m].first += w.n;
      if (M[m].records_left != UNKNOWN) M[m].records_left -= w.n;
      if (M[m].range_left != UNKNOWN) M[m].range_left -= w.n;
      S.records[m] += w.n;
    }
  }
  // What is left of the read streams holds no record -- where the range ends with the archive: behind a range that ends
  // sooner nothing is read, and a stream that is cut short there is not noticed
  int check_end() {
    if (M[m0].range_left == 0 && M[m0].records_left != 0) return SCALCE_OK;
    for (int m = m0; m <= m1; m++) {
      bool more = false;
      SD_TRY(more_reads(m, (size_t)(M[m].L + 3) / 4, more));
      if (more && X && X->taken == X->N)
        return fail(SCALCE_ERR_FORMAT, m0, 4, 0, "(ERROR) order stream holds %llu entries, the archive more records", (unsigned long long)X->N);
      if (more) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) the read stream holds more than the %llu records of the %s stream",
                            (unsigned long long)M[m].first, names ? "name" : "quality");
    }
    return SCALCE_OK;
  }

  // mates m0 .. m1 (one mate, or both under -i) from the range's first window to its last
  int run_pass() {
    const double t_pass = now_s();
    for (int m = m0; m <= m1; m++) SD_TRY(setup_decoder(m));
    if (m1 > m0 && M[m0].records_left != M[m1].records_left)
      return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) the mates hold %llu and %llu records", (unsigned long long)M[m0].records_left,
                  (unsigned long long)M[m1].records_left);
    known = M[m0].records_left != UNKNOWN;
    if (X && known && X->N != M[m0].records_left) return order_count(M[m0].records_left);
    SD_TRY(pass_over());
    for (;;) {
      if (failed) return F.rc;
      Window w;
      SD_TRY(window_records(w));
      if (w.n) SD_TRY(window_fill(w));
      if (!w.n) break;
      SD_TRY(window_upload(w));
      SD_TRY(window_launch(w));
      SD_TRY(window_download(w));
      window_advance(w);
    }
    RS.nrecords = S.records[m0];
    SD_TRY(check_end());
    drain();
    if (failed) return F.rc;
    for (int m = m0; m <= m1; m++) free_decoder(m);
    if (X) {
      if (X->taken != X->N) return order_count(X->taken);
      X->S.group_pass_s += now_s() - t_pass;
      const double tc = now_s();
      SD_TRY(restore_stripes());
      X->S.stripe_pass_s += now_s() - tc;
    }
    return SCALCE_OK;
  }

  int run(scalce_read_fn rd[2][3], void *user[2][3]) {
    const double t0 = now_s();
    SD_HIP(hipGetDevice(&device));
    SD_TRY(headers(rd, user));
    // an archive made with -Q / -f -- a .scalceq that ends behind its header while the read stream holds records -- is an error
    // without -Q: decoding qualities that are not there would misread it
    for (int m = 0; m < P.mates && qual; m++)
      if (M[m].q_empty) {
        bool has = false;
        SD_TRY(more_reads(m, 1, has));
        if (has) return fail(SCALCE_ERR_FORMAT, m, 2, 1, "holds no qualities: the archive was made with -Q or -f; decompress it with -Q");
        M[m].records_left = 0;
      }
    for (Stream *s : {&s_up, &s_main, &s_dec, &s_down}) SD_HIP(s->create());
    writer = std::thread([this] { writer_main(); });
    const bool together = P.mates == 2 && P.interleave;
    for (int m = 0; m < P.mates; m += together ? 2 : 1) {
      m0 = m;
      m1 = together ? 1 : m;
      const double ts = now_s();
      int rc = X ? restore_open(m) : SCALCE_OK;
      if (!rc) rc = setup_slots();
      S.setup_s += now_s() - ts;
      if (!rc) rc = run_pass();
      if (rc) return rc;
      drain();
      free_slots();
    }
    S.total_s = now_s() - t0;
    return SCALCE_OK;
  }

  // The order in which everything goes: the writer is joined (it waits on the slots' events and reads their pinned text), then
  // every stream is synchronised (whatever is still on its way ends before the buffers go), then the buffers and events, and
  // the streams last.
  void close() {
    { std::lock_guard<std::mutex> lk(mu); closing = true; }
    cv.notify_all();
    if (writer.joinable()) writer.join();
    for (Stream *s : {&s_up, &s_main, &s_dec, &s_down}) if (s->s) (void)hipStreamSynchronize(*s);
    for (int m = 0; m < 2; m++) free_decoder(m);
    free_slots();
    for (Stream *s : {&s_up, &s_main, &s_dec, &s_down}) s->release();
  }
};

}  // namespace

// The arithmetic of a range over the coded quality stream, without a device call: symbols [first * L, (first + n) * L) of a
// stream of total_syms symbols in frames of SCALCE_AC_BLOCK.  first and n are clamped to the total_syms / L records the stream
// holds; a range that reaches the last record takes the symbols behind it (fewer than one record) along, as a whole run does.
extern "C" int scalce_range_plan_quality(int read_len, uint64_t first, uint64_t n, uint64_t total_syms, uint64_t out[4]) {
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

extern "C" int scalce_order_plan(uint64_t total_records, uint64_t window_text_bytes, uint64_t max_record_bytes, uint64_t out[2]) {
  if (!out || !max_record_bytes || total_records > 0xFFFFFFFFull) return SCALCE_ERR_ARG;
  scalce_host::order_plan(total_records, window_text_bytes, max_record_bytes, out);
  return SCALCE_OK;
}

extern "C" int scalce_stream_decompress(scalce_ctx *ctx, const scalce_unpack_params *p, scalce_read_fn rd[2][3], void *user[2][3],
                                        scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats, char *errbuf, size_t errcap) {
  return scalce_stream_decompress_range(ctx, p, nullptr, rd, user, wr, wr_user, stats, nullptr, errbuf, errcap);
}

// what every entry point asks of its arguments; the session that runs, reports and goes
static int unpack_args(scalce_ctx *ctx, const scalce_unpack_params *p, scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, char *errbuf,
                       size_t errcap) {
  if (!ctx || !p || !rd || !user || !wr || p->mates < 1 || p->mates > 2 || (p->interleave && p->mates != 2)) return SCALCE_ERR_ARG;
  for (int m = 0; m < p->mates; m++)
    if (!rd[m][0] || !rd[m][1] || (!p->no_qualities && !rd[m][2])) return SCALCE_ERR_ARG;
  if (p->ignore_names && !p->library) return SCALCE_ERR_ARG;
  if ((p->len_rd[0] || p->len_rd[1]) && (p->interleave || p->no_qualities || !p->len_rd[0] || (p->mates == 2 && !p->len_rd[1]))) {
    if (errbuf && errcap)
      snprintf(errbuf, errcap, "(ERROR) a variable-length archive (a length stream) is decompressed one mate after the other, with its qualities: "
                               "not interleaved, not without qualities, and every mate has its length stream");
    return SCALCE_ERR_ARG;
  }
  return SCALCE_OK;
}
static int session_run(Session *s, scalce_read_fn rd[2][3], void *user[2][3], scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats,
                       char *errbuf, size_t errcap) {
  int rc = s->run(rd, user);
  s->close();
  if (!rc && s->failed) rc = s->F.rc;
  if (rc) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", s->F.msg.c_str());
    s->S.error_mate = s->F.mate; s->S.error_stream = s->F.stream; s->S.error_wants_file = s->F.wants_file;
  }
  if (stats) *stats = s->S;
  if (range_stats) *range_stats = s->RS;
  return rc;
}

extern "C" int scalce_stream_decompress_range(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_range *range,
                                              scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                              scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats, char *errbuf,
                                              size_t errcap) {
  if (const int rc = unpack_args(ctx, p, rd, user, wr, errbuf, errcap)) return rc;
  Session *s = new Session(ctx, p, range, wr, wr_user);
  const int rc = session_run(s, rd, user, stats, range_stats, errbuf, errcap);
  delete s;
  return rc;
}

extern "C" int scalce_stream_decompress_restore(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_restore_params *rp,
                                                scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                                scalce_unpack_stats *stats, scalce_restore_stats *restore_stats, char *errbuf, size_t errcap) {
  if (const int rc = unpack_args(ctx, p, rd, user, wr, errbuf, errcap)) return rc;
  if (!rp || !rp->order_rd[0] || (p->mates == 2 && !p->interleave && !rp->order_rd[1])) return SCALCE_ERR_ARG;
  Session *s = new Session(ctx, p, nullptr, wr, wr_user);
  s->X.reset(new Restore);
  s->X->P = *rp;
  memset(&s->X->S, 0, sizeof s->X->S);
  s->X->dir = rp->spill_dir && rp->spill_dir[0] ? rp->spill_dir : ".";
  const int rc = session_run(s, rd, user, stats, nullptr, errbuf, errcap);
  if (restore_stats) *restore_stats = s->X->S;
  delete s;
  return rc;
}
