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
// What is where.  Everything that reads the archive's bytes is host-only and lies in headers that a plain compiler takes:
// archive_walk.hpp (the headers, mate 1's buckets, one function per stream that moves it on by n records -- into the slot or
// to nowhere --, the names, the hop over coded frames, which stream decides the record count, and the reports of a stream that
// ends or fails), over stream_src.hpp (a stream behind its callbacks), lenstream.hpp and orderstream.hpp (the length and the
// order stream, the spill's table, record word and file).  This file holds what needs the device: the Session with its slots,
// the decoder batches, the steps of a window, the writer thread, and the device half of the order restore (Restore).
//
// Built on the public C ABI only (include/scalce_hip.h) plus the HIP runtime for pinned memory, copies and events.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
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
#include "archive_walk.hpp"
#include "hip_own.hpp"
#include "exceptionstream.hpp"
#include "orderstream.hpp"

namespace {

using namespace scalce_host;  // (archive_walk.hpp, orderstream.hpp: the host-only half of this path)

constexpr u64 TABLE_BYTES = 512000ull * 4;
constexpr u64 SCALCE_DECODE_AHEAD = 8;  // windows' worth of symbols per decoder batch

u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

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

// a mate's streams and where the walk stands in them (archive_walk.hpp), and behind them what it holds on the device
struct Mate : ArcMate {
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
  // archives with a comment stream: the window's entries, the text with them put back and what the insert pass works in
  HBuf h_com, h_cbad;
  DBuf d_com, d_textc, d_roffc, d_cws, d_cbad;
  // archives with a plus-line stream: the window's entries, the text with the lines put back and what that pass works in
  HBuf h_plus, h_pbad;
  DBuf d_plus, d_textp, d_roffp, d_pws, d_pbad;
  // archives with an exception stream: the window's entries per mate (they grow with the windows), the verdict, the pairs' scratch
  HBuf h_exc[2], h_xbad;
  DBuf d_exc[2], d_xbad, d_xws;
  // params.digest: the CRC-32 of the text that comes down from this slot (a window's, or a stripe's), and the launch's scratch
  HBuf h_crc;
  DBuf d_crc, d_crcws;
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
  bool com = false;         // the window's entries of the comment stream go back into its text
  u64 cbytes = 0;           // ... their bytes, newlines included
  bool plus = false;        // the window's entries of the plus-line stream go back into its text
  u64 pbytes = 0, pgrow = 0;  // ... their bytes, newlines included, and what they add to the text
  bool exc = false;         // the window's entries of the exception stream go back into its text
  u64 nexc[2] = {0, 0};     // ... how many, per mate
};

struct Job {
  enum Kind { WINDOW, SPILL, STRIPE };  // a window for wr; the order restore: a window for the spill, a stripe for wr
  int slot, mate;
  u64 first, n, nbytes;
  Kind kind;
};

// The order restore (scalce_stream_decompress_restore).  Pass B is the window loop: a window's records are grouped by stripe
// on the device and its text, entries and record sizes appended to the spill by the writer thread.  Pass C reads the spill
// back stripe by stripe, puts the records in their places on the device and hands each stripe to wr.
struct RestoreSlot {
  HBuf h_ord, h_gidx, h_groff, h_counts, h_bad;
  DBuf d_ord, d_sidx, d_gidx, d_gtext, d_groff, d_counts, d_bad, d_ws;
};
struct Session;
struct Restore {
  scalce_restore_params P;
  scalce_restore_stats S;
  Src o;          // the order stream of the pass that runs
  u64 delivered = 0, skipped = 0;
  u64 N = 0, taken = 0;        // entries its header promises; entries the windows have taken
  u64 R = 0, NS = 0;           // records per stripe, stripes (scalce_order_plan)
  u64 rcap = 0;                // records a buffer of record words holds: a window's or a stripe's, whichever is more
  std::string dir;
  SpillFile f_text, f_rec;
  StripeTable table;
  std::vector<u64> words;      // a window's / a stripe's record words (record_word)
  RestoreSlot rs[2];
  // the device half of pass B, step by step of a window (the session's streams, error reports and memory count)
  int setup_slot(Session &s, int i, u64 roff_bytes);
  void free_slots(Session &s);
  int upload(Session &s, const Window &w);
  int group(Session &s, const Window &w, const u8 *d_text, const u64 *d_roff);
  int download(Session &s, const Window &w);
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
  Failure WF;  // what the walk reports (the main thread's alone), on its way into F
  std::atomic<bool> failed{false};
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool closing = false;
  std::thread writer;
  int device = 0;
  std::unique_ptr<Restore> X;  // set: the input order is restored
  scalce_unpack_comments CM;   // the comment streams (scalce_stream_decompress_comments), or none
  u64 cap_com = 0;             // bytes of entries a slot takes
  scalce_unpack_plus PL;       // the plus-line streams (scalce_stream_decompress_plus), or none
  u64 cap_plus = 0;            // bytes of entries a slot takes
  scalce_unpack_exceptions EX; // the exception streams (scalce_stream_decompress_exceptions), or none
  ExceptionCursor xc[2];       // ... where each mate's stands
  bool has_exc[2] = {false, false};
  std::vector<u64> xents;      // a window's entries of one mate, on their way into the slot

  // (the streams in front of what is used on them: close() lets everything go in the right order by hand, and should a
  // session ever die without it, the buffers and events would still go before the streams)
  Stream s_up, s_main, s_dec, s_down;
  Mate M[2];
  Walk A;  // the archive's streams: the pass's mates (m0 .. m1), known, names, qual and the library name are its
  Slot slot[2];
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
    memset(&CM, 0, sizeof CM);
    memset(&EX, 0, sizeof EX);
    memset(&PL, 0, sizeof PL);
    RS.first_record = RG.first_record;
    RS.total_records = UNKNOWN;
    A.M[0] = &M[0];
    A.M[1] = &M[1];
    A.cores.count = scalce_patterns_count(c);
    A.cores.length = [](void *u, int core) { return scalce_pattern_length(static_cast<scalce_ctx *>(u), core); };
    A.cores.string = [](void *u, int core) { return scalce_pattern_string(static_cast<scalce_ctx *>(u), core); };
    A.cores.user = c;
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
  // what a step of the walk (archive_walk.hpp) came back with: its failure, filled into WF, becomes the session's
  int walk(int rc) { return rc ? fail(WF.rc, WF.mate, WF.stream, WF.wants_file, "%s", WF.msg.c_str()) : SCALCE_OK; }
  // ... and a stream that was asked for n records and gave `got`: the one place where a stream that decides the record count
  // (Walk::decides_count) makes n smaller and any other is truncated
  int took(int rc, int m, int stream, const u64 &got, u64 &n) { return walk(rc ? rc : A.ended_at(m, stream, got, n, WF)); }
#define SD_HIP_OF(s, expr) do { if (int rc_ = (s).hip((expr), #expr)) return rc_; } while (0)
#define SD_HIP(expr) SD_HIP_OF(*this, expr)
#define SD_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

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

  // ---- sizes and buffers: from the window, the read lengths and the table, never from the archive --------------------------
  u64 rec_fixed(int m) const { return (A.qual ? 2ull : 1ull) * (u64)M[m].L + (A.qual ? 6 : 3); }
  // text of records [first, first + n) of mate m when names are made up: "<library>.<index>"
  u64 lib_text(int m, u64 first, u64 n, bool with_qual) const {
    auto f = with_qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes;
    return f(M[m].L, first + n, 0, A.library.c_str()) - f(M[m].L, first, 0, A.library.c_str());
  }
  u64 lib_text(int m, u64 first, u64 n) const { return lib_text(m, first, n, A.qual); }

  int setup_slots() {  // mates m0 .. m1 share a window
    W = P.window_text_bytes ? P.window_text_bytes : SCALCE_WINDOW_TEXT_DEFAULT;
    S.window_text_bytes = W;
    u64 rec_min = 0, rec_max = 0;
    // (comment streams: the bound of a record's text grows by the mate's longest entry)
    const bool com = M[A.m0].com.open;
    const u64 nmates = (u64)(A.m1 - A.m0 + 1);
    u64 C = 0;
    for (int m = A.m0; m <= A.m1 && com; m++) C = std::max<u64>(C, M[m].com.longest);
    // (plus-line streams: ... and by the longest a '+' line can become: a literal of P - 1 bytes, or the header line's own bound)
    const bool plus = wants_plus();
    u64 PE = 0;
    for (int m = A.m0; m <= A.m1 && plus; m++) PE = std::max<u64>(PE, M[m].plus.longest);
    for (int m = A.m0; m <= A.m1; m++) {
      const u64 header = 255 + 32 + (com ? M[m].com.longest : 0);
      rec_min += A.rec_budget(m);
      rec_max += rec_fixed(m) + header + (plus ? std::max<u64>(M[m].plus.longest ? M[m].plus.longest - 1 : 0, header) : 0);
    }
    R = std::max<u64>(1, W / rec_min);
    D = std::min<u64>(R, (u64)scalce_patterns_count(ctx) + 2);
    cap_text = std::max(W, rec_max) + 64;
    u64 rcap = R;
    if (X) {  // a stripe's text fits the window's bound, unless the cap on the stripes raised R
      u64 pl[2];
      order_plan(X->N, W, rec_max, pl);
      X->R = pl[0]; X->NS = pl[1];
      X->S.stripe_records = pl[0]; X->S.stripes = pl[1];
      X->table.reset(X->NS);
      cap_text = std::max(cap_text, X->R * rec_max + 64);
      rcap = X->rcap = std::max(R, X->R);
    }
    const u64 roff_bytes = 8 * (rcap + 1), len_bytes = 2 * R + 64;
    u64 o = 0;
    for (int m = A.m0; m <= A.m1; m++) {
      Mate &x = M[m];
      const u64 rb_max = (u64)(x.L + 3) / 4 + 2;
      x.cap_slice = R * rb_max + 12 * D;
      x.o_reads = o; o = align_up(o + x.cap_slice + 64, 256);
      x.o_dir = o; o = align_up(o + sizeof(scalce_fq_bucket) * D, 256);
      if (A.names) {
        x.cap_names = std::min(cap_text, R * 256);
        x.o_names = o; o = align_up(o + x.cap_names + 64, 256);
        x.o_noff = o; o = align_up(o + roff_bytes, 256);
      }
      if (A.qual && x.no_ac) { x.o_qual = o; o = align_up(o + R * (u64)x.L + 64, 256); }
    }
    cap_in = o;
    for (int i = 0; i < 2; i++) {
      Slot &s = slot[i];
      SD_TRY(hmalloc(s.h_in, cap_in));
      SD_TRY(dmalloc(s.d_in, cap_in));
      SD_TRY(hmalloc(s.h_text, cap_text));
      SD_TRY(dmalloc(s.d_text, cap_text));
      const bool strip = M[A.m0].has_len;  // (never with two mates in one window: -d -i refuses a length stream)
      if (P.split) SD_TRY(hmalloc(s.h_roff, roff_bytes));
      const bool exc = has_exc[A.m0];
      if (P.split || strip || X || com || exc || plus) SD_TRY(dmalloc(s.d_roff, roff_bytes));
      if (plus) {  // a window's entries: a repeat or a bare line takes two bytes at most, a literal two more than it adds to the text
        cap_plus = std::min(W + 2 * R * nmates, R * nmates * (PE + 1)) + nmates * (PE + 1) + 64;
        SD_TRY(hmalloc(s.h_plus, cap_plus));
        SD_TRY(hmalloc(s.h_pbad, 64));
        memset(s.h_pbad.p, 0, 64);
        SD_TRY(dmalloc(s.d_plus, cap_plus));
        SD_TRY(dmalloc(s.d_textp, cap_text));
        SD_TRY(dmalloc(s.d_roffp, roff_bytes));
        SD_TRY(dmalloc(s.d_pws, nmates == 2 ? scalce_fastq_plus_pairs_ws_bytes(R, cap_plus) : scalce_fastq_plus_ws_bytes(R, cap_plus)));
        SD_TRY(dmalloc(s.d_pbad, 64));
      }
      if (exc) {
        SD_TRY(hmalloc(s.h_xbad, 64));
        memset(s.h_xbad.p, 0, 64);
        SD_TRY(dmalloc(s.d_xbad, 64));
        if (nmates == 2) SD_TRY(dmalloc(s.d_xws, scalce_fastq_exception_pairs_ws_bytes(R)));
      }
      if (com) {  // a window's entries: no more than its text, nor than its records' times the longest
        cap_com = std::min(std::max(W, nmates * (C + 1)), R * nmates * (C + 1)) + 64;
        SD_TRY(hmalloc(s.h_com, cap_com));
        SD_TRY(hmalloc(s.h_cbad, 64));
        memset(s.h_cbad.p, 0, 64);
        SD_TRY(dmalloc(s.d_com, cap_com));
        SD_TRY(dmalloc(s.d_textc, cap_text));
        SD_TRY(dmalloc(s.d_roffc, roff_bytes));
        SD_TRY(dmalloc(s.d_cws, nmates == 2 ? scalce_fastq_comment_pairs_ws_bytes(R, cap_com) : scalce_fastq_comment_ws_bytes(R, cap_com)));
        SD_TRY(dmalloc(s.d_cbad, 64));
      }
      if (X) SD_TRY(X->setup_slot(*this, i, roff_bytes));
      if (P.digest) {
        SD_TRY(hmalloc(s.h_crc, 64));
        memset(s.h_crc.p, 0, 64);
        SD_TRY(dmalloc(s.d_crc, 64));
        SD_TRY(dmalloc(s.d_crcws, scalce_crc32_ws_bytes(cap_text)));
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
      for (DBuf *b : {&s.d_len, &s.d_text2, &s.d_roff2, &s.d_scan, &s.d_com, &s.d_textc, &s.d_roffc, &s.d_cws, &s.d_cbad, &s.d_exc[0], &s.d_exc[1], &s.d_xbad, &s.d_xws,
                      &s.d_plus, &s.d_textp, &s.d_roffp, &s.d_pws, &s.d_pbad, &s.d_crc, &s.d_crcws,
                      &s.d_in, &s.d_text, &s.d_roff})
        drop(*b);
      s = Slot();
    }
    if (X) X->free_slots(*this);
  }

  // the quality stream behind its header: the table, the symbol count, then the frames -- and the decoder for them
  int setup_decoder(int m) {
    Mate &x = M[m];
    Decoder &d = x.d;
    if (!A.qual || x.no_ac || x.q_empty) return SCALCE_OK;
    std::vector<u32> table(TABLE_BYTES / 4);
    if (x.q.read_into(reinterpret_cast<u8 *>(table.data()), TABLE_BYTES) != TABLE_BYTES) return fail(SCALCE_ERR_FORMAT, m, ST_QUALITY, 0, "(ERROR) truncated quality table");
    if (!x.q.get(x.total_syms)) return walk(truncated(WF, m, ST_QUALITY));
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
      if (!x.q.need(4)) return walk(truncated(WF, m, ST_QUALITY));
      u32 sz;  // (looked at, not taken: a frame that does not fit the staging any more opens the next batch)
      memcpy(&sz, x.q.ptr(), 4);
      if (at + 4 + (u64)sz > d.coded_cap - 64) {
        if (k) break;
        return fail(SCALCE_ERR_FORMAT, m, ST_QUALITY, 0, "(ERROR) a coded block of %u bytes: not a quality stream of this coder", sz);
      }
      memcpy(h_coded + at, &sz, 4);
      x.q.skip(4);
      if (x.q.read_into(h_coded + at + 4, sz) != sz) return walk(truncated(WF, m, ST_QUALITY));
      at += 4 + (u64)sz;
      k++;
    }
    if (x.q.bad) return walk(read_error(WF, m, ST_QUALITY));
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
      if (d.h_bad.as<u32>()[par]) return walk(truncated(WF, m, ST_QUALITY));
    }
  }

  // ---- the writer: one thread, windows in order ----------------------------------------------------------------------------
  // a job's text has come down, and -- the order restore -- its entries were what the header promised; false: the session has failed
  bool text_down(const Job &j) {
    const double t0 = now_s();
    const hipError_t e = hipEventSynchronize(slot[j.slot].ev_done);
    if (e != hipSuccess) hip(e, "a window's text did not come down");
    if (j.kind == Job::STRIPE) X->S.place_wait_s += now_s() - t0;
    if (!failed && j.kind != Job::WINDOW && X->rs[j.slot].h_bad.as<u32>()[0])
      fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "(ERROR) %s", order_not_permutation());
    if (!failed && j.kind != Job::STRIPE && slot[j.slot].h_cbad.p && slot[j.slot].h_cbad.as<u32>()[0])
      fail(SCALCE_ERR_FORMAT, A.m0, ST_COMMENT, 0, "internal: a window's entries of the comment stream do not fit its records");
    if (!failed && j.kind != Job::STRIPE && slot[j.slot].h_pbad.p && slot[j.slot].h_pbad.as<u32>()[0])
      fail(SCALCE_ERR_FORMAT, A.m0, ST_PLUS, 0, "(ERROR) %s", plus_malformed());
    if (!failed && j.kind != Job::STRIPE && slot[j.slot].h_xbad.p && slot[j.slot].h_xbad.as<u32>()[0])
      fail(SCALCE_ERR_FORMAT, A.m0, ST_EXCEPTION, 0, "(ERROR) %s", exception_outside());
    return !failed;
  }
  void records_time(const Slot &s) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.t_rec0, s.t_rec1) == hipSuccess) S.records_s += 1e-3 * ms;
  }
  void hand_over(const Job &j) {
    Slot &s = slot[j.slot];
    const double t0 = now_s();
    if (P.digest) {  // (jobs reach wr in order: so do their words)
      S.crc[j.mate] = scalce_crc32_combine(S.crc[j.mate], s.h_crc.as<u32>()[0], j.nbytes);
      S.text_bytes[j.mate] += j.nbytes;
    }
    if (wr(wr_user, j.mate, j.first, j.n, s.h_text.as<u8>(), j.nbytes, P.split ? s.h_roff.as<u64>() : nullptr)) fail(SCALCE_ERR_FORMAT, j.mate, -1, 0, "the write callback failed");
    S.write_s += now_s() - t0;
  }
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
      if (!failed && text_down(j)) switch (j.kind) {
        case Job::WINDOW: records_time(s); hand_over(j); S.windows++; break;
        case Job::SPILL: records_time(s); spill_window(j); S.windows++; break;
        case Job::STRIPE: hand_over(j); break;
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
  // a slot's text is on its way down (ev_done is recorded): it is the writer's
  void to_writer(int si, u64 first, u64 n, u64 nbytes, Job::Kind kind) {
    {
      std::lock_guard<std::mutex> lk(mu);
      slot[si].busy = true;
      jobs.push_back(Job{si, A.m1 > A.m0 ? 0 : A.m0, first, n, nbytes, kind});
    }
    cv.notify_all();
  }

  // ---- the order restore --------------------------------------------------------------------------------------------------
  int order_count(u64 records) {
    char b[200];
    order_count_message(b, sizeof b, X->N, records);
    return fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "(ERROR) %s", b);
  }
  int spill_error(const char *what) {
    return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) cannot %s a spill file in %s: %s", what, X->dir.c_str(), strerror(errno));
  }
  // a mate pass begins: the order stream from its start, its header, empty spill files
  int restore_open(int m) {
    Restore &x = *X;
    x.o = Src();
    x.o.open(x.P.order_rd[m], nullptr, x.P.order_user[m], &S.read_wait_s, &x.delivered, &x.skipped);
    const bool whole = x.o.need(ORDER_HEADER_BYTES);
    if (x.o.bad) return walk(read_error(WF, m, ST_ORDER));
    if (const char *why = order_header_read(x.o.ptr(), whole ? ORDER_HEADER_BYTES : 0, &x.N))
      return fail(SCALCE_ERR_FORMAT, m, ST_ORDER, 0, "(ERROR) %s", why);
    x.o.skip(ORDER_HEADER_BYTES);
    x.taken = 0;
    for (SpillFile *f : {&x.f_text, &x.f_rec}) {
      const char *what = nullptr;
      if (!f->reset(x.dir, &what)) return spill_error(what);
    }
    return SCALCE_OK;
  }
  bool spill_io(SpillFile &f, bool write, void *p, u64 n, u64 at) {
    const double t0 = now_s();
    const bool ok = f.transfer(write, p, n, at);
    (write ? X->S.spill_write_s : X->S.spill_read_s) += now_s() - t0;
    return ok;
  }
  // (the writer thread) a window's grouped records behind the spill's end; the table learns where its shares lie
  void spill_window(const Job &j) {
    Restore &x = *X;
    const RestoreSlot &q = x.rs[j.slot];
    const u64 *off = q.h_groff.as<u64>();
    const u32 *idx = q.h_gidx.as<u32>();
    const u64 text_at = x.table.text_bytes, rec_at = x.table.records;
    if (off[j.n] - off[0] != j.nbytes || !x.table.add_window(q.h_counts.as<u32>(), off, j.n)) {
      fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "internal: a window's stripes do not add up");
      return;
    }
    x.words.resize(j.n);
    for (u64 k = 0; k < j.n; k++) x.words[k] = record_word(idx[k], off[k + 1] - off[k]);
    if (!spill_io(x.f_text, true, slot[j.slot].h_text.p, j.nbytes, text_at) || !spill_io(x.f_rec, true, x.words.data(), 8 * j.n, 8 * rec_at)) {
      spill_error("write");
      return;
    }
    x.S.spilled_bytes += j.nbytes + 8 * j.n;
  }
  // Pass C: stripe s holds the records of input index [s R, s R + expect).  Every window's share comes back from the spill,
  // goes up, the records find their places and the stripe goes to wr through the writer thread, slot by slot in turn.
  int restore_stripes() {
    Restore &x = *X;
    std::vector<StripeTable::Piece> pieces;
    for (u64 s = 0; s < x.NS; s++) {
      if (failed) return F.rc;
      const u64 base = s * x.R, expect = std::min(x.R, x.N - base);
      u64 bytes = 0;
      const u64 m = x.table.take_stripe(pieces, &bytes);
      if (m != expect) return fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "(ERROR) %s", order_not_permutation());
      if (bytes + 64 > cap_text || m > x.rcap) return fail(SCALCE_ERR_CAPACITY, -1, -1, 0, "internal: a stripe of %llu bytes of text", (unsigned long long)bytes);
      const int si = (int)(s & 1);
      if (!wait_slot(si)) return F.rc;
      Slot &sl = slot[si];
      RestoreSlot &q = x.rs[si];
      x.words.resize(m);
      u64 tb = 0, tr = 0;
      for (const auto &pc : pieces) {
        if (!spill_io(x.f_text, false, sl.h_text.as<u8>() + tb, pc.bytes, pc.text_at) || !spill_io(x.f_rec, false, x.words.data() + tr, 8 * pc.records, 8 * pc.record_at))
          return spill_error("read");
        tb += pc.bytes; tr += pc.records;
      }
      u64 *off = q.h_groff.as<u64>();
      u32 *idx = q.h_ord.as<u32>();
      off[0] = 0;
      for (u64 k = 0; k < m; k++) { idx[k] = record_entry(x.words[k]); off[k + 1] = off[k] + record_size(x.words[k]); }
      if (off[m] != bytes) return fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "internal: a stripe's record sizes do not add up");
      SD_HIP(hipMemcpyAsync(sl.d_text.p, sl.h_text.p, bytes, hipMemcpyHostToDevice, s_main));
      SD_HIP(hipMemcpyAsync(sl.d_roff.p, off, 8 * (m + 1), hipMemcpyHostToDevice, s_main));
      SD_HIP(hipMemcpyAsync(q.d_ord.p, idx, 4 * m, hipMemcpyHostToDevice, s_main));
      SD_TRY(lib(scalce_order_place(ctx, q.d_ord.as<u32>(), m, base, expect, q.d_sidx.as<u32>(), q.d_bad.as<u32>(), s_main)));
      SD_TRY(lib(scalce_records_permute(ctx, sl.d_text.as<u8>(), sl.d_roff.as<u64>(), m, bytes, q.d_sidx.as<u32>(), q.d_gtext.as<u8>(), cap_text,
                                        q.d_groff.as<u64>(), q.d_ws.p, s_main)));
      if (P.digest) {  // the stripe's text where the download reads it
        SD_TRY(lib(scalce_crc32_device(ctx, q.d_gtext.as<u8>(), bytes, sl.d_crc.as<u32>(), sl.d_crcws.p, s_main)));
        SD_HIP(hipMemcpyAsync(sl.h_crc.p, sl.d_crc.p, 4, hipMemcpyDeviceToHost, s_main));
      }
      SD_HIP(hipMemcpyAsync(sl.h_text.p, q.d_gtext.p, bytes, hipMemcpyDeviceToHost, s_main));
      if (P.split) SD_HIP(hipMemcpyAsync(sl.h_roff.p, q.d_groff.p, 8 * (m + 1), hipMemcpyDeviceToHost, s_main));
      SD_HIP(hipMemcpyAsync(q.h_bad.p, q.d_bad.p, 4, hipMemcpyDeviceToHost, s_main));
      SD_HIP(hipEventRecord(sl.ev_done, s_main));
      to_writer(si, base, expect, bytes, Job::STRIPE);
    }
    drain();
    x.S.records = x.N;
    return failed ? F.rc : SCALCE_OK;
  }

  // ---- the range: what lies in front of its first record is passed over, stream by stream -------------------------------
  // Nothing of it reaches the device.  A stream that decides the record count (Walk::decides_count) may end in front of the
  // range, which is empty then.
  int pass_over() {
    const int m0 = A.m0, m1 = A.m1;
    u64 first = RG.first_record, got = 0;
    if (A.known) { RS.total_records = M[m0].records_left; first = std::min(first, M[m0].records_left); }
    for (int m = m0; m <= m1 && A.names; m++) SD_TRY(took(A.pass_names(m, first, got, WF), m, ST_NAME, got, first));
    for (int m = m0; m <= m1; m++)  // -A: rows of L bytes
      if (A.qual && M[m].no_ac) SD_TRY(took(A.quality_rows(m, first, nullptr, got, WF), m, ST_QUALITY, got, first));
    for (int m = m0; m <= m1; m++) SD_TRY(took(A.reads(m, first, nullptr, got, WF), m, ST_READ, got, first));
    for (int m = m0; m <= m1; m++) {  // coded qualities: whole frames by their size words, then the symbols in front of the record
      Mate &x = M[m];
      if (!x.d.dec) continue;
      u64 pl[4];
      if (range_plan_quality(x.L, first, RG.nrecords, x.total_syms, pl)) return fail(SCALCE_ERR_ARG, m, ST_QUALITY, 0, "internal: the range's plan");
      SD_TRY(walk(A.pass_frames(m, pl[0], WF)));
      RS.frames_passed[m] = pl[0];
      x.frames_left = pl[1];
      x.drop = pl[2];
      x.syms_left = pl[2] + pl[3];
    }
    for (int m = m0; m <= m1; m++)  // the length stream: entries of one width
      if (M[m].has_len) SD_TRY(took(A.lengths(m, first, nullptr, got, WF), m, ST_LENGTH, got, first));
    for (int m = m0; m <= m1; m++)  // the comment stream: entries by their newlines
      if (M[m].com.open) SD_TRY(took(A.pass_text(m, M[m].com, first, got, WF), m, ST_COMMENT, got, first));
    for (int m = m0; m <= m1; m++)  // the plus-line stream: the same
      if (M[m].plus.open) SD_TRY(took(A.pass_text(m, M[m].plus, first, got, WF), m, ST_PLUS, got, first));
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      x.first = first;
      x.range_left = RG.nrecords;
      if (A.known) x.records_left -= first;
    }
    RS.first_record = first;
    return SCALCE_OK;
  }

  // ---- the steps of a window, in the order run_pass() takes them ---------------------------------------------------------
  // How many records: what the decoders hold, what the range and the archive leave, then what the text takes -- with names
  // they come into the slot as they are counted, made-up names are bisected.  w.n stays 0: nothing is left
  int window_records(Window &w) {
    const int m0 = A.m0, m1 = A.m1;
    u64 ncap = std::min(R, std::min(M[m0].records_left, M[m0].range_left));
    for (int m = m0; m <= m1 && ncap; m++)
      if (M[m].d.dec) { u64 k; SD_TRY(records_decoded(m, k)); ncap = std::min(ncap, k); }
    if (X) ncap = std::min(ncap, X->N - X->taken);  // (records behind the last entry: check_end reports them)
    if (!ncap) return SCALCE_OK;
    w.si = (int)(widx & 1);
    if (!wait_slot(w.si)) return F.rc;
    w.n = ncap;
    w.first = M[m0].first;
    if (A.names) {
      u8 *h_in = slot[w.si].h_in.as<u8>();
      NamesDst to[2] = {{h_in + M[m0].o_names, reinterpret_cast<u64 *>(h_in + M[m0].o_noff), M[m0].cap_names},
                                     {h_in + M[m1].o_names, reinterpret_cast<u64 *>(h_in + M[m1].o_noff), M[m1].cap_names}};
      CommentsDst cd{slot[w.si].h_com.as<u8>(), cap_com};
      w.com = M[m0].com.open;
      PlusDst pd{slot[w.si].h_plus.as<u8>(), cap_plus};
      w.plus = wants_plus();
      const int rc = A.take_names(to, ncap, W, w.n, w.nb, WF, w.com ? &cd : nullptr, w.plus ? &pd : nullptr);
      w.cbytes = cd.nbytes;
      w.pbytes = pd.nbytes; w.pgrow = pd.grow;
      return walk(rc);
    }
    auto text = [&](u64 k) { u64 t = 0; for (int m = m0; m <= m1; m++) t += lib_text(m, w.first, k, true); return t; };
    if (text(w.n) > W) {
      u64 lo = 1, hi = w.n;  // text(lo) fits (or lo = 1), text(hi) does not
      while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (text(mid) <= W) lo = mid; else hi = mid; }
      w.n = lo;
    }
    w.plus = wants_plus();
    if (w.plus) {  // made-up names: each record's entries are taken with what they add, and the window ends where its budget does
      PlusDst pd{slot[w.si].h_plus.as<u8>(), cap_plus};
      u64 n = 0, t = 0;
      for (; n < w.n; n++) {
        u64 header[2] = {0, 0}, rec = 0;
        for (int m = m0; m <= m1; m++) {
          const u64 one = lib_text(m, w.first + n, 1, true);
          header[m - m0] = one - (2ull * (u64)M[m].L + 6);  // (the record is '@', the name, two lines of L, '+' and four newlines)
          rec += one;
        }
        Walk::PlusPeek pk;
        const int e = A.plus_peek(header, pk, WF);
        if (e == 1 && !A.known) break;  // (the stream ends with the archive, whose other streams say where that is)
        if (e) return walk(e == 1 ? truncated(WF, m0, ST_PLUS) : e);
        if (n && (t + rec + pk.grow > W || !A.plus_fits(pd, pk))) break;
        A.plus_commit(pd, pk);
        t += rec + pk.grow;
      }
      w.n = n;
      w.pbytes = pd.nbytes; w.pgrow = pd.grow;
    }
    return SCALCE_OK;
  }
  // The pinned block from the other streams: raw quality rows, reads, length entries.  A stream that decides the record
  // count may make the window shorter (w.n == 0: the archive ends here); then the text's size is known
  int window_fill(Window &w) {
    const int m0 = A.m0, m1 = A.m1;
    Slot &s = slot[w.si];
    u8 *h_in = s.h_in.as<u8>();
    u64 got = 0;
    for (int m = m0; m <= m1 && w.n; m++)  // -A: the q - offset rows as they are
      if (A.qual && M[m].no_ac) SD_TRY(took(A.quality_rows(m, w.n, h_in + M[m].o_qual, got, WF), m, ST_QUALITY, got, w.n));
    for (int m = m0; m <= m1 && w.n; m++) {
      ReadsDst to{h_in + M[m].o_reads, reinterpret_cast<scalce_fq_bucket *>(h_in + M[m].o_dir), M[m].cap_slice, (u32)D};
      SD_TRY(took(A.reads(m, w.n, &to, got, WF), m, ST_READ, got, w.n));
      w.ndir[m - m0] = to.ndir;
      w.slice[m - m0] = to.bytes;
    }
    if (!w.n) return SCALCE_OK;
    // variable-length: the window's entries; their sum says how much shorter the text comes down than it is made
    w.strip = M[m0].has_len;
    if (w.strip) {
      Mate &x = M[m0];
      SD_TRY(took(A.lengths(m0, w.n, s.h_len.as<u8>(), got, WF), m0, ST_LENGTH, got, w.n));
      const u64 sum = len_entries_sum(s.h_len.as<u8>(), w.n, x.l_width, x.L);
      if (sum == ~0ull) return fail(SCALCE_ERR_FORMAT, m0, ST_LENGTH, 0, "(ERROR) the length stream holds an entry above the read length %d", x.L);
      w.cut = 2 * sum;
    }
    if (X) {  // the window's entries of the order stream
      const u64 want = 4 * w.n;
      if (X->o.read_into(X->rs[w.si].h_ord.as<u8>(), want) != want) return walk(short_stream(WF, m0, ST_ORDER, X->o));
      X->taken += w.n;
    }
    // the exception stream: the entries of the window's records, per mate (the cursor passes over what lies in front of them)
    w.exc = has_exc[m0];
    for (int m = m0; m <= m1 && w.exc; m++) {
      xents.clear();
      if (const char *why = xc[m].take(w.first, w.first + w.n, &xents)) return fail(SCALCE_ERR_FORMAT, m, ST_EXCEPTION, 0, "(ERROR) %s", why);
      const int i = m - m0;
      w.nexc[i] = xents.size();
      if (8 * w.nexc[i] + 64 > s.h_exc[i].cap) {  // (the slot is idle: its last window is written)
        const u64 want = std::max<u64>(2 * s.h_exc[i].cap, 8 * w.nexc[i] + 4096);
        S.pinned_host_bytes -= s.h_exc[i].cap;
        SD_TRY(hmalloc(s.h_exc[i], want));
        drop(s.d_exc[i]);
        SD_TRY(dmalloc(s.d_exc[i], want));
      }
      if (w.nexc[i]) memcpy(s.h_exc[i].p, xents.data(), 8 * w.nexc[i]);
    }
    for (int m = m0; m <= m1; m++)
      w.nbytes += A.names ? (A.qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes)(M[m].L, w.n, w.nb[m - m0], nullptr) : lib_text(m, w.first, w.n);
    if (w.com) w.nbytes += w.cbytes - w.n * (u64)(m1 - m0 + 1);  // (the entries without their newlines)
    if (w.plus) w.nbytes += w.pgrow;
    if (w.nbytes + 64 > cap_text) return fail(SCALCE_ERR_CAPACITY, -1, -1, 0, "internal: a window of %llu bytes of text", (unsigned long long)w.nbytes);
    return SCALCE_OK;
  }
  int window_upload(const Window &w) {
    Slot &s = slot[w.si];
    u8 *h_in = s.h_in.as<u8>(), *d_in = s.d_in.as<u8>();
    if (w.strip) SD_HIP(hipMemcpyAsync(s.d_len.p, s.h_len.p, w.n * (u64)M[A.m0].l_width, hipMemcpyHostToDevice, s_up));
    if (w.com) SD_HIP(hipMemcpyAsync(s.d_com.p, s.h_com.p, w.cbytes, hipMemcpyHostToDevice, s_up));
    if (w.plus && w.pbytes) SD_HIP(hipMemcpyAsync(s.d_plus.p, s.h_plus.p, w.pbytes, hipMemcpyHostToDevice, s_up));
    for (int i = 0; i < 2 && w.exc; i++)
      if (w.nexc[i]) SD_HIP(hipMemcpyAsync(s.d_exc[i].p, s.h_exc[i].p, 8 * w.nexc[i], hipMemcpyHostToDevice, s_up));
    if (X) SD_TRY(X->upload(*this, w));
    for (int m = A.m0; m <= A.m1; m++) {
      Mate &x = M[m];
      const int i = m - A.m0;
      SD_HIP(hipMemcpyAsync(d_in + x.o_reads, h_in + x.o_reads, w.slice[i], hipMemcpyHostToDevice, s_up));
      SD_HIP(hipMemcpyAsync(d_in + x.o_dir, h_in + x.o_dir, sizeof(scalce_fq_bucket) * w.ndir[i], hipMemcpyHostToDevice, s_up));
      if (A.names) {
        SD_HIP(hipMemcpyAsync(d_in + x.o_names, h_in + x.o_names, w.nb[i], hipMemcpyHostToDevice, s_up));
        SD_HIP(hipMemcpyAsync(d_in + x.o_noff, h_in + x.o_noff, 8 * (w.n + 1), hipMemcpyHostToDevice, s_up));
      }
      if (A.qual && x.no_ac) SD_HIP(hipMemcpyAsync(d_in + x.o_qual, h_in + x.o_qual, w.n * (u64)x.L, hipMemcpyHostToDevice, s_up));
    }
    SD_HIP(hipEventRecord(s.ev_up, s_up));
    return SCALCE_OK;
  }
  // where a window's finished text and record offsets lie: behind the strip, else behind the insert, else as the records kernel left them
  DBuf &window_text(const Window &w) { Slot &s = slot[w.si]; return w.plus ? s.d_textp : w.strip ? s.d_text2 : w.com ? s.d_textc : s.d_text; }
  DBuf &window_roff(const Window &w) { Slot &s = slot[w.si]; return w.plus ? s.d_roffp : w.strip ? s.d_roff2 : w.com ? s.d_roffc : s.d_roff; }
  // the plus-line streams are put back: there are some, the records that go out have a third line, and not every line was bare
  bool wants_plus() const {
    bool any = false;
    for (int m = A.m0; m <= A.m1; m++) any = any || (M[m].plus.open && M[m].plus.longest);
    return A.qual && any;
  }
  // records -> text, mate by mate, behind the upload; then the entries come back (comments) and the pad goes (variable-length)
  int window_launch(Window &w) {
    const int m0 = A.m0, m1 = A.m1;
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
      if (A.qual) fw.d_qual = x.no_ac ? d_in + x.o_qual : d.Y[d.cur & 1].as<u8>() + d.pos;
      fw.phred_offset = x.phred;
      if (A.names) { fw.d_names = d_in + x.o_names; fw.d_name_off = reinterpret_cast<const u64 *>(d_in + x.o_noff); }
      fw.library = A.library.c_str();
      fw.d_out = s.d_text.as<u8>();
      fw.d_record_offsets = ((P.split || w.strip || X || w.com || w.exc || w.plus) && m == m0) ? s.d_roff.as<u64>() : nullptr;
      if (nmates == 2) {
        const Mate &y = M[m == m0 ? m1 : m0];
        fw.interleave = m - m0 + 1; fw.pair_read_len = y.L;
        if (A.names) fw.d_pair_name_off = reinterpret_cast<const u64 *>(d_in + y.o_noff);
      }
      SD_TRY(lib(scalce_fastq_records_window(ctx, &fw, s_main)));
      if (d.dec) {
        SD_HIP(hipEventRecord(d.ev_rec[d.cur & 1], s_main));
        d.rec_once[d.cur & 1] = true;
        d.pos += w.n * (u64)x.L;
      }
    }
    // the exceptions first, in place: the comment insert, the strip and the order restore all keep what the lines hold
    if (w.exc && nmates == 2) {
      const int rl[2] = {M[m0].L, M[m1].L};
      const uint64_t *ents[2] = {s.d_exc[0].as<uint64_t>(), s.d_exc[1].as<uint64_t>()};
      SD_TRY(lib(scalce_fastq_exception_window_pairs(ctx, rl, A.qual ? 1 : 0, w.first, w.n, s.d_text.as<u8>(), s.d_roff.as<u64>(),
                                                     A.names ? reinterpret_cast<const u64 *>(d_in + M[m1].o_noff) : nullptr, A.library.size(), ents,
                                                     w.nexc, s.d_xbad.as<u32>(), s.d_xws.p, s_main)));
    } else if (w.exc)
      SD_TRY(lib(scalce_fastq_exception_window(ctx, M[m0].L, A.qual ? 1 : 0, w.first, w.n, s.d_text.as<u8>(), s.d_roff.as<u64>(),
                                               s.d_exc[0].as<uint64_t>(), w.nexc[0], s.d_xbad.as<u32>(), s_main)));
    // the entries go back in BEFORE the strip (which measures from the record's end) and before the order restore groups the
    // window (its records are self-contained text)
    if (w.com && nmates == 2) {  // (one interleaved text: both mates' entries, pair by pair)
      const int rl[2] = {M[m0].L, M[m1].L};
      SD_TRY(lib(scalce_fastq_comment_window_pairs(ctx, rl, A.qual ? 1 : 0, w.n, s.d_text.as<u8>(), s.d_roff.as<u64>(),
                                                   reinterpret_cast<const u64 *>(d_in + M[m1].o_noff), s.d_com.as<u8>(), w.cbytes, s.d_textc.as<u8>(),
                                                   s.d_roffc.as<u64>(), s.d_cbad.as<u32>(), s.d_cws.p, s_main)));
    } else if (w.com)
      SD_TRY(lib(scalce_fastq_comment_window(ctx, M[m0].L, A.qual ? 1 : 0, w.n, s.d_text.as<u8>(), s.d_roff.as<u64>(), s.d_com.as<u8>(), w.cbytes,
                                             s.d_textc.as<u8>(), s.d_roffc.as<u64>(), s.d_cbad.as<u32>(), s.d_cws.p, s_main)));
    if (w.strip) {  // the text and its record offsets come down from the stripped copy
      SD_TRY(lib(scalce_fastq_strip_window(ctx, M[m0].L, w.n, (w.com ? s.d_textc : s.d_text).as<u8>(), (w.com ? s.d_roffc : s.d_roff).as<u64>(),
                                           s.d_len.as<u8>(), M[m0].l_width, s.d_text2.as<u8>(), s.d_roff2.as<u64>(), s.d_scan.p, s_main)));
      w.nbytes -= w.cut;
    }
    // the '+' lines go back BEHIND the comment insert and the strip: both measure from the record's end and assume "\n+\n"
    if (w.plus) {
      DBuf &src = w.strip ? s.d_text2 : w.com ? s.d_textc : s.d_text, &src_off = w.strip ? s.d_roff2 : w.com ? s.d_roffc : s.d_roff;
      if (nmates == 2) {
        const int rl[2] = {M[m0].L, M[m1].L};
        SD_TRY(lib(scalce_fastq_plus_window_pairs(ctx, rl, w.n, src.as<u8>(), src_off.as<u64>(), s.d_plus.as<u8>(), w.pbytes, s.d_textp.as<u8>(),
                                                  cap_text, s.d_roffp.as<u64>(), s.d_pbad.as<u32>(), s.d_pws.p, s_main)));
      } else
        SD_TRY(lib(scalce_fastq_plus_window(ctx, w.n, src.as<u8>(), src_off.as<u64>(), s.d_plus.as<u8>(), w.pbytes, s.d_textp.as<u8>(), cap_text,
                                            s.d_roffp.as<u64>(), s.d_pbad.as<u32>(), s.d_pws.p, s_main)));
    }
    if (X) SD_TRY(X->group(*this, w, window_text(w).as<u8>(), window_roff(w).as<u64>()));
    SD_HIP(hipEventRecord(s.t_rec1, s_main));
    SD_HIP(hipEventRecord(s.ev_rec, s_main));
    return SCALCE_OK;
  }
  // the text comes down behind the kernels; the writer gets the window
  int window_download(const Window &w) {
    Slot &s = slot[w.si];
    SD_HIP(hipStreamWaitEvent(s_down, s.ev_rec, 0));
    if (X) {
      SD_TRY(X->download(*this, w));
    } else {
      if (P.digest) {  // the window's final text where the download reads it
        SD_TRY(lib(scalce_crc32_device(ctx, window_text(w).as<u8>(), w.nbytes, s.d_crc.as<u32>(), s.d_crcws.p, s_down)));
        SD_HIP(hipMemcpyAsync(s.h_crc.p, s.d_crc.p, 4, hipMemcpyDeviceToHost, s_down));
      }
      SD_HIP(hipMemcpyAsync(s.h_text.p, window_text(w).p, w.nbytes, hipMemcpyDeviceToHost, s_down));
      if (P.split) SD_HIP(hipMemcpyAsync(s.h_roff.p, window_roff(w).p, 8 * (w.n + 1), hipMemcpyDeviceToHost, s_down));
    }
    if (w.com) SD_HIP(hipMemcpyAsync(s.h_cbad.p, s.d_cbad.p, 4, hipMemcpyDeviceToHost, s_down));
    if (w.exc) SD_HIP(hipMemcpyAsync(s.h_xbad.p, s.d_xbad.p, 4, hipMemcpyDeviceToHost, s_down));
    if (w.plus) SD_HIP(hipMemcpyAsync(s.h_pbad.p, s.d_pbad.p, 4, hipMemcpyDeviceToHost, s_down));
    SD_HIP(hipEventRecord(s.ev_done, s_down));
    to_writer(w.si, w.first, w.n, w.nbytes, X ? Job::SPILL : Job::WINDOW);
    return SCALCE_OK;
  }
  void window_advance(const Window &w) {
    widx++;
    for (int m = A.m0; m <= A.m1; m++) {
      M[m].first += w.n;
      if (M[m].records_left != UNKNOWN) M[m].records_left -= w.n;
      if (M[m].range_left != UNKNOWN) M[m].range_left -= w.n;
      S.records[m] += w.n;
    }
  }
  // What is left of the read streams holds no record (Walk::reads_at_end says where that is looked at, and where not)
  int check_end() {
    int more = -1;
    SD_TRY(walk(A.reads_at_end(more, WF)));
    if (more < 0) return SCALCE_OK;
    if (X && X->taken == X->N)
      return fail(SCALCE_ERR_FORMAT, A.m0, ST_ORDER, 0, "(ERROR) order stream holds %llu entries, the archive more records", (unsigned long long)X->N);
    return walk(A.holds_more(more, WF));
  }

  // mates m0 .. m1 (one mate, or both under -i) from the range's first window to its last
  int run_pass() {
    const int m0 = A.m0, m1 = A.m1;
    const double t_pass = now_s();
    for (int m = m0; m <= m1; m++) SD_TRY(setup_decoder(m));
    if (m1 > m0 && M[m0].records_left != M[m1].records_left)
      return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) the mates hold %llu and %llu records", (unsigned long long)M[m0].records_left,
                  (unsigned long long)M[m1].records_left);
    A.known = M[m0].records_left != UNKNOWN;
    if (X && A.known && X->N != M[m0].records_left) return order_count(M[m0].records_left);
    for (int m = m0; m <= m1; m++)
      if (M[m].com.open && A.known && M[m].com.total != M[m0].records_left) return walk(A.text_count(m, M[m].com, M[m].com.total, M[m0].records_left, WF));
    for (int m = m0; m <= m1; m++)
      if (M[m].plus.open && A.known && M[m].plus.total != M[m0].records_left) return walk(A.text_count(m, M[m].plus, M[m].plus.total, M[m0].records_left, WF));
    for (int m = m0; m <= m1; m++) {
      if (!has_exc[m]) continue;
      char b[200];
      if (A.known && xc[m].records != M[m0].records_left) {
        exception_count_message(b, sizeof b, xc[m].records, M[m0].records_left);
        return fail(SCALCE_ERR_FORMAT, m, ST_EXCEPTION, 0, "(ERROR) %s", b);
      }
      if (xc[m].read_len != (uint32_t)M[m].L) {
        exception_length_message(b, sizeof b, xc[m].read_len, (uint32_t)M[m].L);
        return fail(SCALCE_ERR_FORMAT, m, ST_EXCEPTION, 0, "(ERROR) %s", b);
      }
    }
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
    // (an archive that does not say how many records it holds, read to its end: the stream must have ended with it)
    for (int m = m0; m <= m1; m++)
      if (M[m].com.open && M[m0].range_left == UNKNOWN && M[m].com.taken != M[m].com.total) return walk(A.text_count(m, M[m].com, M[m].com.total, M[m].com.taken, WF));
    for (int m = m0; m <= m1; m++)
      if (M[m].plus.open && M[m].plus.longest && M[m0].range_left == UNKNOWN && M[m].plus.taken != M[m].plus.total) return walk(A.text_count(m, M[m].plus, M[m].plus.total, M[m].plus.taken, WF));
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
    SD_TRY(walk(A.headers(P, RG, rd, user, &S.read_wait_s, RS, WF)));
    // an archive made with -Q / -f -- a .scalceq that ends behind its header while the read stream holds records -- is an error
    // without -Q: decoding qualities that are not there would misread it
    for (int m = 0; m < P.mates && A.qual; m++)
      if (M[m].q_empty) {
        bool has = false;
        SD_TRY(walk(A.more_reads(m, 1, has, WF)));
        if (has) return fail(SCALCE_ERR_FORMAT, m, ST_QUALITY, 1, "holds no qualities: the archive was made with -Q or -f; decompress it with -Q");
        M[m].records_left = 0;
      }
    for (int m = 0; m < P.mates; m++) {  // the comment streams: header, then one entry per record
      if (!CM.com_rd[m]) continue;
      if (!A.names) return fail(SCALCE_ERR_ARG, m, ST_COMMENT, 0, "(ERROR) a comment stream goes with stored names: the archive holds none (or -n sets them aside)");
      SD_TRY(walk(A.text_open(m, M[m].com, CM.com_rd[m], CM.com_user[m], &S.read_wait_s, WF)));
    }
    for (int m = 0; m < P.mates; m++) {  // the plus-line streams: header, then one entry per record (none when P = 0)
      if (!PL.plus_rd[m]) continue;
      if (!A.qual) return fail(SCALCE_ERR_ARG, m, ST_PLUS, 0, "(ERROR) a plus-line stream goes with four-line records: -Q writes two");
      SD_TRY(walk(A.text_open(m, M[m].plus, PL.plus_rd[m], PL.plus_user[m], &S.read_wait_s, WF)));
    }
    for (int m = 0; m < P.mates; m++) {  // the exception streams: header, then the entries in ascending order
      if (!EX.exc_rd[m]) continue;
      xc[m].start(EX.exc_rd[m], EX.exc_user[m]);
      if (const char *why = xc[m].read_header()) return fail(SCALCE_ERR_FORMAT, m, ST_EXCEPTION, 0, "(ERROR) %s", why);
      has_exc[m] = true;
    }
    for (Stream *s : {&s_up, &s_main, &s_dec, &s_down}) SD_HIP(s->create());
    writer = std::thread([this] { writer_main(); });
    const bool together = P.mates == 2 && P.interleave;
    for (int m = 0; m < P.mates; m += together ? 2 : 1) {
      A.m0 = m;
      A.m1 = together ? 1 : m;
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

// ---- the device half of the order restore's pass B ---------------------------------------------------------------------------
int Restore::setup_slot(Session &s, int i, u64 roff_bytes) {
  RestoreSlot &q = rs[i];
  const u64 words = 4 * rcap + 64, ws = std::max(scalce_order_group_ws_bytes(rcap, NS), scalce_records_permute_ws_bytes(rcap));
  for (HBuf *b : {&q.h_ord, &q.h_gidx}) SD_TRY(s.hmalloc(*b, words));
  SD_TRY(s.hmalloc(q.h_groff, roff_bytes));
  SD_TRY(s.hmalloc(q.h_counts, 4 * NS + 64));
  SD_TRY(s.hmalloc(q.h_bad, 64));
  for (DBuf *b : {&q.d_ord, &q.d_sidx, &q.d_gidx}) SD_TRY(s.dmalloc(*b, words));
  SD_TRY(s.dmalloc(q.d_gtext, s.cap_text));
  SD_TRY(s.dmalloc(q.d_groff, roff_bytes));
  SD_TRY(s.dmalloc(q.d_counts, 4 * NS + 64));
  SD_TRY(s.dmalloc(q.d_bad, 64));
  return s.dmalloc(q.d_ws, ws);
}
void Restore::free_slots(Session &s) {
  for (RestoreSlot &q : rs) {
    for (DBuf *b : {&q.d_ord, &q.d_sidx, &q.d_gidx, &q.d_gtext, &q.d_groff, &q.d_counts, &q.d_bad, &q.d_ws}) s.drop(*b);
    q = RestoreSlot();
  }
}
// the window's entries of the order stream go up with the rest of it
int Restore::upload(Session &s, const Window &w) {
  SD_HIP_OF(s, hipMemcpyAsync(rs[w.si].d_ord.p, rs[w.si].h_ord.p, 4 * w.n, hipMemcpyHostToDevice, s.s_up));
  return SCALCE_OK;
}
// behind the text: the window's records grouped by the stripe of the output they belong to, and their entries with them
int Restore::group(Session &s, const Window &w, const u8 *d_text, const u64 *d_roff) {
  RestoreSlot &q = rs[w.si];
  SD_TRY(s.lib(scalce_order_group(s.ctx, q.d_ord.as<u32>(), w.n, R, N, NS, q.d_sidx.as<u32>(), q.d_counts.as<u32>(), q.d_bad.as<u32>(), q.d_ws.p, s.s_main)));
  SD_TRY(s.lib(scalce_records_permute(s.ctx, d_text, d_roff, w.n, w.nbytes, q.d_sidx.as<u32>(), q.d_gtext.as<u8>(), s.cap_text, q.d_groff.as<u64>(),
                                      q.d_ws.p, s.s_main)));
  return s.lib(scalce_order_gather(s.ctx, q.d_ord.as<u32>(), q.d_sidx.as<u32>(), w.n, q.d_gidx.as<u32>(), s.s_main));
}
// what comes down: the grouped text, where its records begin, their entries, the stripes' counts and the verdict
int Restore::download(Session &s, const Window &w) {
  RestoreSlot &q = rs[w.si];
  SD_HIP_OF(s, hipMemcpyAsync(s.slot[w.si].h_text.p, q.d_gtext.p, w.nbytes, hipMemcpyDeviceToHost, s.s_down));
  SD_HIP_OF(s, hipMemcpyAsync(q.h_groff.p, q.d_groff.p, 8 * (w.n + 1), hipMemcpyDeviceToHost, s.s_down));
  SD_HIP_OF(s, hipMemcpyAsync(q.h_gidx.p, q.d_gidx.p, 4 * w.n, hipMemcpyDeviceToHost, s.s_down));
  SD_HIP_OF(s, hipMemcpyAsync(q.h_counts.p, q.d_counts.p, 4 * NS, hipMemcpyDeviceToHost, s.s_down));
  SD_HIP_OF(s, hipMemcpyAsync(q.h_bad.p, q.d_bad.p, 4, hipMemcpyDeviceToHost, s.s_down));
  return SCALCE_OK;
}

}  // namespace

extern "C" int scalce_range_plan_quality(int read_len, uint64_t first, uint64_t n, uint64_t total_syms, uint64_t out[4]) {
  return scalce_host::range_plan_quality(read_len, first, n, total_syms, out);
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

// the three shapes of decompression behind one call, with or without comment streams (the entry points below and above are this)
static int decompress_any(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *cm, const scalce_unpack_exceptions *ex,
                          const scalce_unpack_plus *pl,
                          const scalce_unpack_range *range, const scalce_restore_params *rp, scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                          scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats, scalce_restore_stats *restore_stats, char *errbuf,
                          size_t errcap) {
  if (const int rc = unpack_args(ctx, p, rd, user, wr, errbuf, errcap)) return rc;
  if (rp && (range || !rp->order_rd[0] || (p->mates == 2 && !p->interleave && !rp->order_rd[1]))) return SCALCE_ERR_ARG;
  const bool com = cm && (cm->com_rd[0] || cm->com_rd[1]);
  if (com && (!cm->com_rd[0] || (p->mates == 2 && !cm->com_rd[1]))) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "(ERROR) an archive with comment streams: every mate has its stream");
    return SCALCE_ERR_ARG;
  }
  const bool exc = ex && (ex->exc_rd[0] || ex->exc_rd[1]);
  if (exc && (!ex->exc_rd[0] || (p->mates == 2 && !ex->exc_rd[1]))) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "(ERROR) an archive with exception streams: every mate has its stream");
    return SCALCE_ERR_ARG;
  }
  const bool plus = pl && (pl->plus_rd[0] || pl->plus_rd[1]);
  if (plus && (!pl->plus_rd[0] || (p->mates == 2 && !pl->plus_rd[1]))) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "(ERROR) an archive with plus-line streams: every mate has its stream");
    return SCALCE_ERR_ARG;
  }
  Session *s = new Session(ctx, p, range, wr, wr_user);
  if (plus) s->PL = *pl;
  if (com) s->CM = *cm;
  if (exc) s->EX = *ex;
  if (rp) {
    s->X.reset(new Restore);
    s->X->P = *rp;
    memset(&s->X->S, 0, sizeof s->X->S);
    s->X->dir = rp->spill_dir && rp->spill_dir[0] ? rp->spill_dir : ".";
  }
  const int rc = session_run(s, rd, user, stats, rp ? nullptr : range_stats, errbuf, errcap);
  if (rp && restore_stats) *restore_stats = s->X->S;
  delete s;
  return rc;
}
extern "C" int scalce_stream_decompress_comments(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments,
                                                 const scalce_unpack_range *range, const scalce_restore_params *rp, scalce_read_fn rd[2][3],
                                                 void *user[2][3], scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats,
                                                 scalce_unpack_range_stats *range_stats, scalce_restore_stats *restore_stats, char *errbuf,
                                                 size_t errcap) {
  return decompress_any(ctx, p, comments, nullptr, nullptr, range, rp, rd, user, wr, wr_user, stats, range_stats, restore_stats, errbuf, errcap);
}
extern "C" int scalce_stream_decompress_exceptions(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments,
                                                   const scalce_unpack_exceptions *exceptions, const scalce_unpack_range *range,
                                                   const scalce_restore_params *rp, scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr,
                                                   void *wr_user, scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats,
                                                   scalce_restore_stats *restore_stats, char *errbuf, size_t errcap) {
  return decompress_any(ctx, p, comments, exceptions, nullptr, range, rp, rd, user, wr, wr_user, stats, range_stats, restore_stats, errbuf, errcap);
}
extern "C" int scalce_stream_decompress_plus(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments,
                                             const scalce_unpack_exceptions *exceptions, const scalce_unpack_plus *plus,
                                             const scalce_unpack_range *range, const scalce_restore_params *rp, scalce_read_fn rd[2][3],
                                             void *user[2][3], scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats,
                                             scalce_unpack_range_stats *range_stats, scalce_restore_stats *restore_stats, char *errbuf,
                                             size_t errcap) {
  return decompress_any(ctx, p, comments, exceptions, plus, range, rp, rd, user, wr, wr_user, stats, range_stats, restore_stats, errbuf, errcap);
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
