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

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/scalce_hip.h"
#include "lenstream.hpp"

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u64 FRAME = SCALCE_AC_BLOCK;
constexpr u64 TABLE_BYTES = 512000ull * 4;
constexpr u64 SCALCE_DECODE_AHEAD = 8;  // windows' worth of symbols per decoder batch
constexpr u64 UNKNOWN = ~0ull;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

// one stream of the archive behind its read callback: a look-ahead buffer for the parts the host walks (headers, names,
// frame sizes), bulk reads straight into the caller's pinned memory for the rest
struct Src {
  scalce_read_fn rd = nullptr;
  scalce_skip_fn skp = nullptr;
  void *user = nullptr;
  std::vector<u8> buf;
  size_t pos = 0, end = 0;
  bool eof = false, bad = false;
  double *wait = nullptr;
  u64 *delivered = nullptr, *skipped = nullptr;
  void open(scalce_read_fn f, scalce_skip_fn sk, void *u, double *w, u64 *del, u64 *skd) {
    rd = f; skp = f ? sk : nullptr; user = u; wait = w; delivered = del; skipped = skd;
    buf.resize(SCALCE_UNPACK_LOOKAHEAD_BYTES);
  }
  size_t avail() const { return end - pos; }
  const u8 *ptr() const { return buf.data() + pos; }
  void skip(size_t n) { pos += n; }
  int64_t pull(void *dst, u64 cap) {
    if (!rd) { eof = true; return 0; }
    const double t0 = now_s();
    const int64_t k = rd(user, dst, cap);
    *wait += now_s() - t0;
    if (k < 0) bad = true;
    if (k == 0) eof = true;
    if (k > 0) *delivered += (u64)k;
    return k;
  }
  // false: the stream ends (or fails) before n bytes.  `look`: how far a refill may read ahead of the n bytes asked for --
  // the whole buffer for a stream that is read from end to end; less in front of bytes that are about to be passed over
  bool need(size_t n, size_t look = ~(size_t)0) { return end - pos >= n ? true : fill(n, look); }
  bool fill(size_t n, size_t look) {
    if (pos) { memmove(buf.data(), buf.data() + pos, end - pos); end -= pos; pos = 0; }
    if (buf.size() < n) buf.resize(n);
    while (end < n && !eof && !bad) {
      const int64_t k = pull(buf.data() + end, std::min(buf.size() - end, n - end + std::min(look, buf.size())));
      if (k > 0) end += (size_t)k;
    }
    return end >= n;
  }
  // passes over n bytes: what the look-ahead buffer holds first, then the caller's skip, or -- without one -- reads that are
  // dropped; returns the bytes passed over (< n: the stream ends there, or has failed)
  u64 pass(u64 n) {
    u64 got = std::min<u64>(n, avail());
    pos += got;
    if (got < n && skp && !eof && !bad) {
      const double t0 = now_s();
      const int64_t k = skp(user, n - got);
      *wait += now_s() - t0;
      if (k < 0 || (u64)k > n - got) bad = true;
      else { got += (u64)k; *skipped += (u64)k; if (got < n) eof = true; }
      return got;
    }
    while (got < n && !eof && !bad) {
      pos = end = 0;
      const int64_t k = pull(buf.data(), std::min<u64>(buf.size(), n - got));
      if (k > 0) got += (u64)k;
    }
    return got;
  }
  // n bytes into dst: what the buffer holds first, then the callback directly; returns the bytes delivered (< n: the end)
  u64 read_into(u8 *dst, u64 n) {
    u64 got = std::min<u64>(n, avail());
    memcpy(dst, ptr(), got);
    pos += got;
    while (got < n && !eof && !bad) {
      const int64_t k = pull(dst + got, n - got);
      if (k > 0) got += (u64)k;
    }
    return got;
  }
};

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
  // the arithmetic decoder: batches of whole frames ahead of the windows
  scalce_ac_decoder *dec = nullptr;
  u64 frames_left = 0, syms_left = 0;
  u64 G = 0, ycap = 0, coded_cap = 0;
  u8 *Y[2] = {nullptr, nullptr}, *d_coded[2] = {nullptr, nullptr}, *h_coded = nullptr;
  u64 *d_off[2] = {nullptr, nullptr};
  u32 *d_size[2] = {nullptr, nullptr};  // G sizes and the walk's verdict behind them
  u32 *h_bad = nullptr;                 // pinned, one word per parity
  hipEvent_t ev_coded_up = nullptr, ev_dec[2] = {nullptr, nullptr}, ev_rec[2] = {nullptr, nullptr}, t_dec0[2] = {nullptr, nullptr},
             t_dec1[2] = {nullptr, nullptr};
  bool coded_up_once = false, rec_once[2] = {false, false};
  u64 have_b[2] = {0, 0};     // symbols a batch buffer holds, carry included
  int64_t enq = -1, cur = -1;  // last batch enqueued, batch being consumed
  u64 pos = 0;                // consumed of the current batch
  // where this mate's parts of a window lie in the slot's input block
  u64 o_reads = 0, o_dir = 0, o_names = 0, o_noff = 0, o_qual = 0;
  u64 cap_slice = 0, cap_names = 0;
};

struct Slot {
  u8 *h_in = nullptr, *d_in = nullptr, *h_text = nullptr, *d_text = nullptr;
  u64 *h_roff = nullptr, *d_roff = nullptr;
  // variable-length archives: the window's entries of the length stream, and what strips the pad off its text
  u8 *h_len = nullptr, *d_len = nullptr, *d_text2 = nullptr;
  u64 *d_roff2 = nullptr;
  void *d_scan = nullptr;
  hipEvent_t ev_up = nullptr, ev_rec = nullptr, ev_done = nullptr, t_rec0 = nullptr, t_rec1 = nullptr;
  bool busy = false;
};

struct Job {
  int slot, mate;
  u64 first, n, nbytes;
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

  Mate M[2];
  Slot slot[2];
  hipStream_t s_up = nullptr, s_main = nullptr, s_dec = nullptr, s_down = nullptr;
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

  template <class T> int dmalloc(T **p, u64 bytes) {
    SD_HIP(hipMalloc(reinterpret_cast<void **>(p), bytes));
    live += bytes;
    S.peak_device_bytes = std::max(S.peak_device_bytes, live);
    return SCALCE_OK;
  }
  template <class T> void dfree(T *&p, u64 bytes) { if (p) { hipFree(p); live -= bytes; p = nullptr; } }
  template <class T> int hmalloc(T **p, u64 bytes) {
    SD_HIP(hipHostMalloc(reinterpret_cast<void **>(p), bytes, hipHostMallocDefault));
    S.pinned_host_bytes += bytes;
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
        if (!x.r.need(4)) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
        memcpy(&v, x.r.ptr(), 4); x.r.skip(4);
        x.no_ac = v;
      }
      if (!x.r.need(4)) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
      memcpy(&v, x.r.ptr(), 4); x.r.skip(4);
      x.L = v;
      if (x.L <= 0) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) read length %d in the read stream's header", x.L);
      if (x.r.bad) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "read error on the read stream");
      if (qual) {
        if (x.q.need(16)) { memcpy(&x.phred, x.q.ptr() + 8, 8); x.q.skip(16); } else x.q.skip(x.q.avail());
        x.q_empty = !x.q.need(1);
        if (x.q.bad) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "read error on the quality stream");
      }
      if (x.n.need(8)) x.n.skip(8);
      if (P.len_rd[m]) {  // the fourth stream: header, then one entry per record
        x.l.open(P.len_rd[m], P.len_skip[m], P.len_user[m], &S.read_wait_s, &x.l_delivered, &x.l_skipped);
        int hl = 0;
        const bool whole = x.l.need(scalce_host::LEN_HEADER_BYTES);
        if (x.l.bad) return fail(SCALCE_ERR_FORMAT, m, 3, 0, "read error on the length stream");
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
        if (x.r.bad) { fail(SCALCE_ERR_FORMAT, m, 0, 0, "read error on the read stream"); return -1; }
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

  int setup_slots(int m0, int m1) {  // mates m0 .. m1 share a window (one mate, or both under -i)
    W = P.window_text_bytes ? P.window_text_bytes : SCALCE_WINDOW_TEXT_DEFAULT;
    S.window_text_bytes = W;
    u64 rec_min = 0, rec_max = 0;
    for (int m = m0; m <= m1; m++) { rec_min += rec_budget(m); rec_max += rec_fixed(m) + 255 + 32; }
    R = std::max<u64>(1, W / rec_min);
    D = std::min<u64>(R, (u64)scalce_patterns_count(ctx) + 2);
    cap_text = std::max(W, rec_max) + 64;
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
        x.o_noff = o; o = align_up(o + 8 * (R + 1), 256);
      }
      if (qual && x.no_ac) { x.o_qual = o; o = align_up(o + R * (u64)x.L + 64, 256); }
    }
    cap_in = o;
    for (int i = 0; i < 2; i++) {
      Slot &s = slot[i];
      SD_TRY(hmalloc(&s.h_in, cap_in));
      SD_TRY(dmalloc(&s.d_in, cap_in));
      SD_TRY(hmalloc(&s.h_text, cap_text));
      SD_TRY(dmalloc(&s.d_text, cap_text));
      const bool strip = M[m0].has_len;  // (never with two mates in one window: -d -i refuses a length stream)
      if (P.split) SD_TRY(hmalloc(&s.h_roff, 8 * (R + 1)));
      if (P.split || strip) SD_TRY(dmalloc(&s.d_roff, 8 * (R + 1)));
      if (strip) {
        SD_TRY(hmalloc(&s.h_len, 2 * R + 64));
        SD_TRY(dmalloc(&s.d_len, 2 * R + 64));
        SD_TRY(dmalloc(&s.d_text2, cap_text));
        SD_TRY(dmalloc(&s.d_roff2, 8 * (R + 1)));
        SD_TRY(dmalloc(&s.d_scan, scalce_fastq_strip_ws_bytes(R)));
      }
      SD_HIP(hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming));
      SD_HIP(hipEventCreateWithFlags(&s.ev_rec, hipEventDisableTiming));
      SD_HIP(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
      SD_HIP(hipEventCreate(&s.t_rec0));
      SD_HIP(hipEventCreate(&s.t_rec1));
    }
    return SCALCE_OK;
  }
  void free_slots() {
    for (int i = 0; i < 2; i++) {
      Slot &s = slot[i];
      if (s.h_in) hipHostFree(s.h_in);
      if (s.h_text) hipHostFree(s.h_text);
      if (s.h_roff) hipHostFree(s.h_roff);
      if (s.h_len) hipHostFree(s.h_len);
      dfree(s.d_len, 2 * R + 64);
      dfree(s.d_text2, cap_text);
      dfree(s.d_roff2, 8 * (R + 1));
      dfree(s.d_scan, scalce_fastq_strip_ws_bytes(R));
      dfree(s.d_in, cap_in);
      dfree(s.d_text, cap_text);
      dfree(s.d_roff, 8 * (R + 1));
      for (hipEvent_t e : {s.ev_up, s.ev_rec, s.ev_done, s.t_rec0, s.t_rec1}) if (e) hipEventDestroy(e);
      s = Slot();
    }
  }

  // the quality stream behind its header: the table, the symbol count, then the frames -- and the decoder for them
  int setup_decoder(int m) {
    Mate &x = M[m];
    if (!qual || x.no_ac || x.q_empty) return SCALCE_OK;
    std::vector<u32> table(TABLE_BYTES / 4);
    if (x.q.read_into(reinterpret_cast<u8 *>(table.data()), TABLE_BYTES) != TABLE_BYTES) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality table");
    if (!x.q.need(8)) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
    memcpy(&x.total_syms, x.q.ptr(), 8);
    x.q.skip(8);
    x.records_left = x.total_syms / (u64)x.L;
    x.syms_left = x.total_syms;
    x.frames_left = (x.total_syms + FRAME - 1) / FRAME;
    SD_TRY(lib(scalce_ac_decoder_create(ctx, table.data(), s_dec, &x.dec)));
    live += scalce_ac_decoder_device_bytes(x.dec);
    S.peak_device_bytes = std::max(S.peak_device_bytes, live);
    x.G = std::max<u64>(1, (SCALCE_DECODE_AHEAD * R * (u64)x.L + FRAME - 1) / FRAME);
    x.ycap = (u64)x.L + x.G * FRAME + 256;
    // a frame of quality strings codes to a third of its symbols; a batch whose frames do not fit the staging is cut short
    // (at least one frame: a single frame larger than this is not an archive of this coder)
    x.coded_cap = std::max<u64>(x.G * FRAME / 2, FRAME * 2) + 4096;
    SD_TRY(hmalloc(&x.h_coded, x.coded_cap));
    SD_TRY(hmalloc(&x.h_bad, 2 * sizeof(u32)));
    SD_HIP(hipEventCreateWithFlags(&x.ev_coded_up, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
      SD_TRY(dmalloc(&x.Y[i], x.ycap));
      SD_TRY(dmalloc(&x.d_coded[i], x.coded_cap));
      SD_TRY(dmalloc(&x.d_off[i], 8 * x.G));
      SD_TRY(dmalloc(&x.d_size[i], 4 * (x.G + 1)));
      SD_HIP(hipEventCreateWithFlags(&x.ev_dec[i], hipEventDisableTiming));
      SD_HIP(hipEventCreateWithFlags(&x.ev_rec[i], hipEventDisableTiming));
      SD_HIP(hipEventCreate(&x.t_dec0[i]));
      SD_HIP(hipEventCreate(&x.t_dec1[i]));
    }
    return SCALCE_OK;
  }
  void free_decoder(int m) {
    Mate &x = M[m];
    if (x.dec) { live -= scalce_ac_decoder_device_bytes(x.dec); scalce_ac_decoder_destroy(x.dec); x.dec = nullptr; }
    if (x.h_coded) hipHostFree(x.h_coded);
    if (x.h_bad) hipHostFree(x.h_bad);
    x.h_coded = nullptr; x.h_bad = nullptr;
    if (x.ev_coded_up) hipEventDestroy(x.ev_coded_up);
    x.ev_coded_up = nullptr;
    for (int i = 0; i < 2; i++) {
      dfree(x.Y[i], x.ycap);
      dfree(x.d_coded[i], x.coded_cap);
      dfree(x.d_off[i], 8 * x.G);
      dfree(x.d_size[i], 4 * (x.G + 1));
      for (hipEvent_t *e : {&x.ev_dec[i], &x.ev_rec[i], &x.t_dec0[i], &x.t_dec1[i]}) { if (*e) hipEventDestroy(*e); *e = nullptr; }
    }
  }

  // ---- the decoder's batches ---------------------------------------------------------------------------------------------
  // Batch b = the next whole frames of mate m, up to G of them, decoded into Y[b & 1] behind what batch b - 1 leaves over:
  // windows take whole records, so that carry is have(b - 1) mod L bytes, known before batch b - 1 has been decoded.  Called
  // when the windows of batch b - 2 have all been enqueued: their last records kernel is what the buffer waits for.
  int enqueue_batch(int m) {
    Mate &x = M[m];
    if (!x.frames_left) return SCALCE_OK;
    const int64_t b = x.enq + 1;
    const int par = (int)(b & 1);
    if (x.coded_up_once) SD_HIP(hipEventSynchronize(x.ev_coded_up));  // the staging's previous bytes have gone up
    u64 at = 0;
    u32 k = 0;
    while (k < x.G && k < x.frames_left) {
      if (!x.q.need(4)) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
      u32 sz;
      memcpy(&sz, x.q.ptr(), 4);
      if (at + 4 + (u64)sz > x.coded_cap - 64) {
        if (k) break;
        return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) a coded block of %u bytes: not a quality stream of this coder", sz);
      }
      memcpy(x.h_coded + at, &sz, 4);
      x.q.skip(4);
      if (x.q.read_into(x.h_coded + at + 4, sz) != sz) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
      at += 4 + (u64)sz;
      k++;
    }
    if (x.q.bad) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "read error on the quality stream");
    const u64 nsym = std::min<u64>((u64)k * FRAME, x.syms_left);
    // (the first batch of a range begins with x.drop symbols of the records in front of it: they are left where they are
    // decoded and the windows begin behind them, so the carry counts from there)
    const u64 carry = b ? (x.have_b[par ^ 1] - (b == 1 ? x.drop : 0)) % (u64)x.L : 0;
    if (x.rec_once[par]) SD_HIP(hipStreamWaitEvent(s_dec, x.ev_rec[par], 0));
    SD_HIP(hipMemcpyAsync(x.d_coded[par], x.h_coded, at, hipMemcpyHostToDevice, s_dec));
    SD_HIP(hipEventRecord(x.ev_coded_up, s_dec));
    x.coded_up_once = true;
    if (carry) SD_HIP(hipMemcpyAsync(x.Y[par], x.Y[par ^ 1] + x.have_b[par ^ 1] - carry, carry, hipMemcpyDeviceToDevice, s_dec));
    SD_HIP(hipEventRecord(x.t_dec0[par], s_dec));
    SD_TRY(lib(scalce_ac_decoder_launch(x.dec, x.d_coded[par], at, k, nsym, x.d_off[par], x.d_size[par], x.d_size[par] + x.G, x.Y[par] + carry, s_dec)));
    SD_HIP(hipEventRecord(x.t_dec1[par], s_dec));
    SD_HIP(hipMemcpyAsync(&x.h_bad[par], x.d_size[par] + x.G, sizeof(u32), hipMemcpyDeviceToHost, s_dec));
    SD_HIP(hipEventRecord(x.ev_dec[par], s_dec));
    x.have_b[par] = carry + nsym;
    x.frames_left -= k;
    x.syms_left -= nsym;
    x.enq = b;
    S.decode_batches[m]++;
    RS.frames_decoded[m] += k;
    RS.symbols_decoded[m] += nsym;
    return SCALCE_OK;
  }
  // whole records of mate m that the decoded symbols still hold; moves on to the next batch when that is none
  int records_decoded(int m, u64 &n) {
    Mate &x = M[m];
    const u64 L = (u64)x.L;
    for (;;) {  // (a range's first batch may hold less than one record behind the symbols it drops: then the next one)
      if (x.cur >= 0 && (x.have_b[x.cur & 1] - x.pos) / L) { n = (x.have_b[x.cur & 1] - x.pos) / L; return SCALCE_OK; }
      if (x.cur == x.enq && !x.frames_left) { n = 0; return SCALCE_OK; }
      if (x.enq == x.cur) SD_TRY(enqueue_batch(m));
      x.cur++;
      x.pos = x.cur ? 0 : x.drop;
      SD_TRY(enqueue_batch(m));  // the batch behind it: decoded while this one's windows go through
      const int par = (int)(x.cur & 1);
      SD_HIP(hipEventSynchronize(x.ev_dec[par]));
      float ms = 0;
      SD_HIP(hipEventElapsedTime(&ms, x.t_dec0[par], x.t_dec1[par]));
      S.decode_s += 1e-3 * ms;
      if (x.h_bad[par]) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
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
        const hipError_t e = hipEventSynchronize(s.ev_done);
        if (e != hipSuccess) hip(e, "a window's text did not come down");
      }
      if (!failed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.t_rec0, s.t_rec1) == hipSuccess) S.records_s += 1e-3 * ms;
        const double t0 = now_s();
        if (wr(wr_user, j.mate, j.first, j.n, s.h_text, j.nbytes, P.split ? s.h_roff : nullptr)) fail(SCALCE_ERR_FORMAT, j.mate, -1, 0, "the write callback failed");
        S.write_s += now_s() - t0;
        S.windows++;
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

  // ---- one window --------------------------------------------------------------------------------------------------------
  // names of up to `ncap` records (pairs) into the slot, as many as the window's text takes; n = how many
  int take_names(Slot &s, int m0, int m1, u64 ncap, bool known, u64 &n, u64 nb[2]) {
    u64 text = 0;
    nb[0] = nb[1] = 0;
    n = 0;
    u64 *noff[2] = {reinterpret_cast<u64 *>(s.h_in + M[m0].o_noff), reinterpret_cast<u64 *>(s.h_in + M[m1].o_noff)};
    u8 *dst[2] = {s.h_in + M[m0].o_names, s.h_in + M[m1].o_names};
    const int nmates = m1 - m0 + 1;
    while (n < ncap) {
      u32 len[2] = {0, 0};
      int ended = 0;
      u64 rec = 0;
      for (int i = 0; i < nmates; i++) {
        Src &src = M[m0 + i].n;
        if (!src.need(1)) { ended++; continue; }
        len[i] = src.ptr()[0];
        if (!src.need(1 + (size_t)len[i])) return fail(SCALCE_ERR_FORMAT, m0 + i, 1, 0, "(ERROR) truncated name stream");
        rec += len[i] + rec_budget(m0 + i);
      }
      if (ended) {
        for (int i = 0; i < nmates; i++) if (M[m0 + i].n.bad) return fail(SCALCE_ERR_FORMAT, m0 + i, 1, 0, "read error on the name stream");
        if (known || ended != nmates) return fail(SCALCE_ERR_FORMAT, m0, 1, 0, "(ERROR) truncated name stream");
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
    u8 *dst = s.h_in + x.o_reads;
    scalce_fq_bucket *dir = reinterpret_cast<scalce_fq_bucket *>(s.h_in + x.o_dir);
    got = 0; ndir = 0; slice = 0;
    if (m != 0) {  // bare records in mate 1's order
      const u64 rb = (u64)(x.L + 3) / 4;
      const u64 bytes = x.r.read_into(dst, n * rb);
      if (x.r.bad) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "read error on the read stream");
      got = bytes / rb;
      if (bytes % rb) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
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
      if (x.r.read_into(dst + slice, bytes) != bytes) return fail(SCALCE_ERR_FORMAT, m, 0, 0, x.r.bad ? "read error on the read stream" : "(ERROR) truncated read stream");
      scalce_fq_bucket &b = dir[ndir++];
      memset(&b, 0, sizeof b);
      b.first = got; b.off = slice; b.core_len = x.bk.core_len; b.rec_bytes = x.bk.rec_bytes;
      memcpy(b.core, x.bk.core, x.bk.core_len);
      slice += bytes; got += t; x.bk.left -= t;
    }
    return SCALCE_OK;
  }

  // ---- the range: what lies in front of its first record is passed over, stream by stream -------------------------------
  // Nothing of it reaches the device.  Where no symbol count says how many records the archive holds, the streams that end it
  // for a whole run -- the names, else the raw quality rows, else the read stream -- end it here too: a range that begins
  // behind them is empty.  Any other stream that ends in front of the range is truncated, as it is for a whole run.
  int pass_over(int m0, int m1) {
    const bool known = M[m0].records_left != UNKNOWN;
    u64 first = RG.first_record;
    if (known) { RS.total_records = M[m0].records_left; first = std::min(first, M[m0].records_left); }
    constexpr size_t LOOK = 64u << 10;  // read ahead of a bucket header when the bucket behind it is skipped, not read
    if (names)  // a length byte per name has to be read: the names go through the look-ahead buffer, not through skip
      for (int m = m0; m <= m1; m++) {
        Src &src = M[m].n;
        u64 k = 0;
        for (; k < first && src.need(1); k++) {
          const size_t len = src.ptr()[0];
          if (!src.need(1 + len)) return fail(SCALCE_ERR_FORMAT, m, 1, 0, src.bad ? "read error on the name stream" : "(ERROR) truncated name stream");
          src.skip(1 + len);
        }
        if (src.bad) return fail(SCALCE_ERR_FORMAT, m, 1, 0, "read error on the name stream");
        if (k < first) {
          if (known || m != m0) return fail(SCALCE_ERR_FORMAT, m, 1, 0, "(ERROR) truncated name stream");
          first = k;
        }
      }
    for (int m = m0; m <= m1; m++) {  // -A: rows of L bytes
      Mate &x = M[m];
      if (!qual || !x.no_ac) continue;
      const u64 want = first * (u64)x.L, bytes = x.q.pass(want);
      if (x.q.bad) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "read error on the quality stream");
      if (bytes != want) {
        if (known || names || m != m0 || bytes % (u64)x.L) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
        first = bytes / (u64)x.L;
      }
    }
    for (int m = m0; m <= m1; m++) {
      Mate &x = M[m];
      u64 got = 0;
      if (m != 0) {
        const u64 rb = (u64)(x.L + 3) / 4, bytes = x.r.pass(first * rb);
        if (bytes % rb && !x.r.bad) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
        got = bytes / rb;
      } else {
        while (got < first) {  // bucket by bucket: every header is read and checked, the records behind it are not
          if (!x.bk.left) {
            const int e = next_bucket(m, x.r.skp ? LOOK : ~(size_t)0);
            if (e < 0) return F.rc;
            if (e) break;
          }
          const u64 t = std::min(x.bk.left, first - got), bytes = t * x.bk.rec_bytes;
          if (x.r.pass(bytes) != bytes) return fail(SCALCE_ERR_FORMAT, m, 0, 0, x.r.bad ? "read error on the read stream" : "(ERROR) truncated read stream");
          got += t; x.bk.left -= t;
        }
      }
      if (x.r.bad) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "read error on the read stream");
      if (got != first) {
        if (known || names || m != m0 || (qual && x.no_ac)) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
        first = got;
      }
    }
    for (int m = m0; m <= m1; m++) {  // coded qualities: whole frames by their size words, then the symbols in front of the record
      Mate &x = M[m];
      if (!x.dec) continue;
      u64 pl[4];
      if (scalce_range_plan_quality(x.L, first, RG.nrecords, x.total_syms, pl)) return fail(SCALCE_ERR_ARG, m, 2, 0, "internal: the range's plan");
      for (u64 f = 0; f < pl[0]; f++) {
        if (!x.q.need(4, x.q.skp ? 0 : ~(size_t)0)) return fail(SCALCE_ERR_FORMAT, m, 2, 0, x.q.bad ? "read error on the quality stream" : "(ERROR) truncated quality stream");
        u32 sz;
        memcpy(&sz, x.q.ptr(), 4);
        x.q.skip(4);
        if (x.q.pass(sz) != sz) return fail(SCALCE_ERR_FORMAT, m, 2, 0, x.q.bad ? "read error on the quality stream" : "(ERROR) truncated quality stream");
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
      if (x.l.pass(want) != want) return fail(SCALCE_ERR_FORMAT, m, 3, 0, x.l.bad ? "read error on the length stream" : "(ERROR) truncated length stream");
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

  // mates m0 .. m1 (one mate, or both under -i) from the range's first window to its last
  int run_pass(int m0, int m1) {
    const int nmates = m1 - m0 + 1;
    for (int m = m0; m <= m1; m++) SD_TRY(setup_decoder(m));
    if (nmates == 2 && M[m0].records_left != M[m1].records_left)
      return fail(SCALCE_ERR_FORMAT, -1, -1, 0, "(ERROR) the mates hold %llu and %llu records", (unsigned long long)M[m0].records_left,
                  (unsigned long long)M[m1].records_left);
    const bool known = M[m0].records_left != UNKNOWN;
    SD_TRY(pass_over(m0, m1));
    for (;;) {
      if (failed) return F.rc;
      u64 ncap = std::min(R, std::min(M[m0].records_left, M[m0].range_left));
      for (int m = m0; m <= m1 && ncap; m++)
        if (M[m].dec) { u64 k; SD_TRY(records_decoded(m, k)); ncap = std::min(ncap, k); }
      if (!ncap) break;
      const int si = (int)(widx & 1);
      Slot &s = slot[si];
      if (!wait_slot(si)) return F.rc;
      // how many records: what the text takes, then what the streams hold
      u64 n = ncap, nb[2] = {0, 0};
      const u64 first = M[m0].first;
      if (names) SD_TRY(take_names(s, m0, m1, ncap, known, n, nb));
      else {
        auto text = [&](u64 k) { u64 t = 0; for (int m = m0; m <= m1; m++) t += lib_text(m, first, k, true); return t; };
        if (text(n) > W) {
          u64 lo = 1, hi = n;  // text(lo) fits (or lo = 1), text(hi) does not
          while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (text(mid) <= W) lo = mid; else hi = mid; }
          n = lo;
        }
      }
      for (int m = m0; m <= m1 && n; m++) {  // -A: the q - offset rows as they are
        Mate &x = M[m];
        if (!qual || !x.no_ac) continue;
        const u64 bytes = x.q.read_into(s.h_in + x.o_qual, n * (u64)x.L);
        if (x.q.bad) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "read error on the quality stream");
        if (bytes != n * (u64)x.L) {
          if (names || m != m0 || bytes % (u64)x.L) return fail(SCALCE_ERR_FORMAT, m, 2, 0, "(ERROR) truncated quality stream");
          n = bytes / (u64)x.L;  // made-up names: this stream says how many records there are
        }
      }
      u32 ndir[2] = {0, 0};
      u64 slice[2] = {0, 0};
      for (int m = m0; m <= m1 && n; m++) {
        u64 got = 0;
        SD_TRY(take_reads(s, m, n, got, ndir[m - m0], slice[m - m0]));
        if (got != n) {
          if (known || names || m != m0 || (qual && M[m].no_ac)) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) truncated read stream");
          n = got;  // no qualities, made-up names: the read stream says how many records there are
        }
      }
      if (!n) break;
      // variable-length: the window's entries; their sum says how much shorter the text comes down than it is made
      const bool strip = M[m0].has_len;
      u64 cut = 0;
      if (strip) {
        Mate &x = M[m0];
        const u64 want = n * (u64)x.l_width;
        if (x.l.read_into(s.h_len, want) != want)
          return fail(SCALCE_ERR_FORMAT, m0, 3, 0, x.l.bad ? "read error on the length stream" : "(ERROR) truncated length stream");
        const u64 sum = scalce_host::len_entries_sum(s.h_len, n, x.l_width, x.L);
        if (sum == ~0ull) return fail(SCALCE_ERR_FORMAT, m0, 3, 0, "(ERROR) the length stream holds an entry above the read length %d", x.L);
        cut = 2 * sum;
        SD_HIP(hipMemcpyAsync(s.d_len, s.h_len, want, hipMemcpyHostToDevice, s_up));
      }
      // up, records -> text, down
      u64 nbytes = 0;
      for (int m = m0; m <= m1; m++)
        nbytes += names ? (qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes)(M[m].L, n, nb[m - m0], nullptr) : lib_text(m, first, n);
      if (nbytes + 64 > cap_text) return fail(SCALCE_ERR_CAPACITY, -1, -1, 0, "internal: a window of %llu bytes of text", (unsigned long long)nbytes);
      for (int m = m0; m <= m1; m++) {
        Mate &x = M[m];
        const int i = m - m0;
        SD_HIP(hipMemcpyAsync(s.d_in + x.o_reads, s.h_in + x.o_reads, slice[i], hipMemcpyHostToDevice, s_up));
        SD_HIP(hipMemcpyAsync(s.d_in + x.o_dir, s.h_in + x.o_dir, sizeof(scalce_fq_bucket) * ndir[i], hipMemcpyHostToDevice, s_up));
        if (names) {
          SD_HIP(hipMemcpyAsync(s.d_in + x.o_names, s.h_in + x.o_names, nb[i], hipMemcpyHostToDevice, s_up));
          SD_HIP(hipMemcpyAsync(s.d_in + x.o_noff, s.h_in + x.o_noff, 8 * (n + 1), hipMemcpyHostToDevice, s_up));
        }
        if (qual && x.no_ac) SD_HIP(hipMemcpyAsync(s.d_in + x.o_qual, s.h_in + x.o_qual, n * (u64)x.L, hipMemcpyHostToDevice, s_up));
      }
      SD_HIP(hipEventRecord(s.ev_up, s_up));
      SD_HIP(hipStreamWaitEvent(s_main, s.ev_up, 0));
      SD_HIP(hipEventRecord(s.t_rec0, s_main));
      for (int m = m0; m <= m1; m++) {
        Mate &x = M[m];
        scalce_fq_window w;
        memset(&w, 0, sizeof w);
        w.d_reads = s.d_in + x.o_reads;
        w.d_dir = reinterpret_cast<const scalce_fq_bucket *>(s.d_in + x.o_dir);
        w.nbuckets = ndir[m - m0];
        w.read_len = x.L; w.has_buckets = m == 0; w.mate_digit = P.mate_digit ? '1' + m : 0;
        w.nrecords = n; w.first_record = first;
        if (qual) w.d_qual = x.no_ac ? s.d_in + x.o_qual : x.Y[x.cur & 1] + x.pos;
        w.phred_offset = x.phred;
        if (names) { w.d_names = s.d_in + x.o_names; w.d_name_off = reinterpret_cast<const u64 *>(s.d_in + x.o_noff); }
        w.library = library.c_str();
        w.d_out = s.d_text;
        w.d_record_offsets = ((P.split || strip) && m == m0) ? s.d_roff : nullptr;
        if (nmates == 2) {
          const Mate &y = M[m == m0 ? m1 : m0];
          w.interleave = m - m0 + 1; w.pair_read_len = y.L;
          if (names) w.d_pair_name_off = reinterpret_cast<const u64 *>(s.d_in + y.o_noff);
        }
        SD_TRY(lib(scalce_fastq_records_window(ctx, &w, s_main)));
        if (x.dec) {
          SD_HIP(hipEventRecord(x.ev_rec[x.cur & 1], s_main));
          x.rec_once[x.cur & 1] = true;
          x.pos += n * (u64)x.L;
        }
      }
      if (strip) {  // the pad goes: the text and its record offsets come down from the stripped copy
        SD_TRY(lib(scalce_fastq_strip_window(ctx, M[m0].L, n, s.d_text, s.d_roff, s.d_len, M[m0].l_width, s.d_text2, s.d_roff2, s.d_scan, s_main)));
        nbytes -= cut;
      }
      SD_HIP(hipEventRecord(s.t_rec1, s_main));
      SD_HIP(hipEventRecord(s.ev_rec, s_main));
      SD_HIP(hipStreamWaitEvent(s_down, s.ev_rec, 0));
      SD_HIP(hipMemcpyAsync(s.h_text, strip ? s.d_text2 : s.d_text, nbytes, hipMemcpyDeviceToHost, s_down));
      if (P.split) SD_HIP(hipMemcpyAsync(s.h_roff, strip ? s.d_roff2 : s.d_roff, 8 * (n + 1), hipMemcpyDeviceToHost, s_down));
      SD_HIP(hipEventRecord(s.ev_done, s_down));
      {
        std::lock_guard<std::mutex> lk(mu);
        s.busy = true;
        jobs.push_back(Job{si, nmates == 2 ? 0 : m0, first, n, nbytes});
      }
      cv.notify_all();
      widx++;
      for (int m = m0; m <= m1; m++) {
        M[m].first += n;
        if (M[m].records_left != UNKNOWN) M[m].records_left -= n;
        if (M[m].range_left != UNKNOWN) M[m].range_left -= n;
        S.records[m] += n;
      }
    }
    RS.nrecords = S.records[m0];
    // what is left of the read streams holds no record -- where the range ends with the archive: behind a range that ends
    // sooner nothing is read, and a stream that is cut short there is not noticed
    const bool to_end = M[m0].range_left != 0 || M[m0].records_left == 0;
    for (int m = m0; m <= m1 && to_end; m++) {
      Mate &x = M[m];
      bool more = false;
      if (m == 0) { const int e = x.bk.left ? 0 : next_bucket(m); if (e < 0) return F.rc; more = e == 0; }
      else more = x.r.need((size_t)(x.L + 3) / 4);
      if (more) return fail(SCALCE_ERR_FORMAT, m, 0, 0, "(ERROR) the read stream holds more than the %llu records of the %s stream",
                            (unsigned long long)x.first, names ? "name" : "quality");
    }
    drain();
    if (failed) return F.rc;
    for (int m = m0; m <= m1; m++) free_decoder(m);
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
        if (m == 0) { const int e = next_bucket(0); if (e < 0) return F.rc; has = e == 0; }
        else has = M[m].r.need(1);
        if (has) return fail(SCALCE_ERR_FORMAT, m, 2, 1, "holds no qualities: the archive was made with -Q or -f; decompress it with -Q");
        M[m].records_left = 0;
      }
    SD_HIP(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
    SD_HIP(hipStreamCreateWithFlags(&s_main, hipStreamNonBlocking));
    SD_HIP(hipStreamCreateWithFlags(&s_dec, hipStreamNonBlocking));
    SD_HIP(hipStreamCreateWithFlags(&s_down, hipStreamNonBlocking));
    writer = std::thread([this] { writer_main(); });
    const bool together = P.mates == 2 && P.interleave;
    for (int m = 0; m < P.mates; m += together ? 2 : 1) {
      const int m1 = together ? 1 : m;
      const double ts = now_s();
      int rc = setup_slots(m, m1);
      S.setup_s += now_s() - ts;
      if (!rc) rc = run_pass(m, m1);
      if (rc) return rc;
      drain();
      free_slots();
    }
    S.total_s = now_s() - t0;
    return SCALCE_OK;
  }

  void close() {
    { std::lock_guard<std::mutex> lk(mu); closing = true; }
    cv.notify_all();
    if (writer.joinable()) writer.join();
    // whatever is still on its way ends before the buffers go
    for (hipStream_t s : {s_up, s_main, s_dec, s_down}) if (s) (void)hipStreamSynchronize(s);
    for (int m = 0; m < 2; m++) free_decoder(m);
    free_slots();
    for (hipStream_t s : {s_up, s_main, s_dec, s_down}) if (s) hipStreamDestroy(s);
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

extern "C" int scalce_stream_decompress(scalce_ctx *ctx, const scalce_unpack_params *p, scalce_read_fn rd[2][3], void *user[2][3],
                                        scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats, char *errbuf, size_t errcap) {
  return scalce_stream_decompress_range(ctx, p, nullptr, rd, user, wr, wr_user, stats, nullptr, errbuf, errcap);
}

extern "C" int scalce_stream_decompress_range(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_range *range,
                                              scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                              scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats, char *errbuf,
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
  Session *s = new Session(ctx, p, range, wr, wr_user);
  int rc = s->run(rd, user);
  s->close();
  if (!rc && s->failed) rc = s->F.rc;
  if (rc) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", s->F.msg.c_str());
    s->S.error_mate = s->F.mate; s->S.error_stream = s->F.stream; s->S.error_wants_file = s->F.wants_file;
  }
  if (stats) *stats = s->S;
  if (range_stats) *range_stats = s->RS;
  delete s;
  return rc;
}
