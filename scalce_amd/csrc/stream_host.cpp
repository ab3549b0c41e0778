// stream_host.cpp -- streaming host of the compress path: files of any size through one GPU.
//
// What it replaces in the reference: the reader half of thread() (compress.cpp:614-671: records read one by one under
// r_spin from zlib-backed files) together with the reason for the spill files (compress.cpp:708-715: the bucket pool is
// bounded).  Here the TEXT is what is bounded: reader threads (one per mate) fill pinned chunks, the chunks go up with
// hipMemcpyAsync while the previous piece is ingested / counted / tokenized (scalce_batch_append), and only the rows
// derived from the text stay in HBM.  Order, emit and entropy then run once over the whole run, so the archive is the one
// a single resident shard gives -- and -B chunks are cut on run-wide record sizes exactly like the reference's.
//
// Built on the public C ABI only (include/scalce_hip.h) plus the HIP runtime for pinned memory and copies.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/scalce_hip.h"
#include "hip_own.hpp"

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// pinned chunks of one mate's stream: filled by the reader thread, drained by the upload
struct ChunkRing {
  struct Chunk {
    uint8_t *p = nullptr;
    uint64_t n = 0;
    bool last = false;  // nothing behind this chunk
  };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Chunk> free_, full_;
  std::string error;
  bool failed = false, stop = false;

  Chunk take_free() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !free_.empty() || stop; });
    if (stop) return Chunk();
    Chunk c = free_.front();
    free_.pop_front();
    return c;
  }
  void put_full(const Chunk &c) {
    { std::lock_guard<std::mutex> lk(mu); full_.push_back(c); }
    cv.notify_all();
  }
  bool take_full(Chunk &c) {  // false: the reader failed
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !full_.empty() || failed; });
    if (full_.empty()) return false;
    c = full_.front();
    full_.pop_front();
    return true;
  }
  void put_free(const Chunk &c) {
    { std::lock_guard<std::mutex> lk(mu); free_.push_back(c); }
    cv.notify_all();
  }
  void fail(const std::string &msg) {
    { std::lock_guard<std::mutex> lk(mu); failed = true; error = msg; }
    cv.notify_all();
  }
  void shutdown() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
  }
};

void reader_main(ChunkRing *ring, scalce_read_fn rd, void *user, uint64_t piece) {
  for (;;) {
    ChunkRing::Chunk c = ring->take_free();
    if (!c.p) return;
    c.n = 0;
    c.last = false;
    while (c.n < piece) {
      const int64_t k = rd(user, c.p + c.n, piece - c.n);
      if (k < 0) { ring->fail("read error on the input stream"); return; }
      if (k == 0) { c.last = true; break; }
      c.n += (uint64_t)k;
    }
    ring->put_full(c);
    if (c.last) return;
  }
}

struct Mate {
  ChunkRing ring;
  std::thread reader;
  std::vector<HBuf> pinned;  // (the ring's chunks: they go only after the reader has been joined)
  // the piece handed to the batch: [tail of the previous piece][new chunks]; two buffers, so that the tail moves to the
  // front of the OTHER one (no overlapping copy)
  DBuf d_text[2];
  int cur = 0;
  uint64_t have = 0;              // bytes of d_text[cur] in use
  // chunks on their way up: a queue of at most two, slot = index & 1
  DBuf d_raw[2];
  uint64_t raw_n[2] = {0, 0};
  Event up_ev[2];    // the chunk has arrived in d_raw[slot]
  Event land_ev[2];  // ... and has been copied behind the tail: the slot may be overwritten
  bool landed_once[2] = {false, false};
  ChunkRing::Chunk raw_chunk[2];
  uint64_t head = 0, tail = 0;    // queue of chunks in d_raw: [head, tail)
  bool eof = false;               // the stream's last chunk has been taken from the ring
  bool all_landed() const { return eof && head == tail; }
  // SCALCE_STREAM_DIGEST: a ring of CRC words, one per chunk, each with the event behind its way down; `open` = chunks whose word
  // has not been joined yet (slot, bytes), oldest first
  static constexpr int CRC_SLOTS = 64;
  DBuf d_crc, d_crc_ws;
  HBuf h_crc;
  std::vector<Event> crc_ev;
  std::deque<std::pair<int, uint64_t>> crc_open;
  uint64_t crc_chunks = 0;
  uint32_t crc = 0;
  uint8_t *text() const { return d_text[cur].as<uint8_t>(); }
};

#define ST_HIP(expr)                                                                                              \
  do {                                                                                                            \
    hipError_t e_ = (expr);                                                                                       \
    if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return SCALCE_ERR_HIP; }     \
  } while (0)

// The run itself.  Whatever it returns, the caller joins the readers, lets the buffers, events and streams go and, on an
// error, puts `err` into errbuf and destroys the batch: nothing is cleaned up in here.
int stream_run(scalce_ctx *ctx, const scalce_params *p, scalce_read_fn rd[2], void *user[2], int nm, uint64_t piece, uint64_t reads_hint,
               int flags, Stream &s_copy, Stream &s_main, Mate M[2], scalce_batch *&b, scalce_stream_stats &S, std::string &err) {
  const int NPIN = 3;
  const uint64_t cap = 2 * piece;  // of a piece: the tail of the previous one plus one chunk
  int rc = SCALCE_OK;
  ST_HIP(s_copy.create());
  ST_HIP(s_main.create());
  for (int m = 0; m < nm; m++) {
    for (int i = 0; i < NPIN; i++) {
      M[m].pinned.emplace_back();
      ST_HIP(M[m].pinned.back().alloc(piece));
      ChunkRing::Chunk c;
      c.p = M[m].pinned.back().as<uint8_t>();
      M[m].ring.free_.push_back(c);
    }
    for (int i = 0; i < 2; i++) {
      ST_HIP(dbuf_alloc(M[m].d_text[i], cap + 256));
      ST_HIP(dbuf_alloc(M[m].d_raw[i], piece + 256));
      ST_HIP(M[m].up_ev[i].create());
      ST_HIP(M[m].land_ev[i].create());
    }
  }
  {
    const uint64_t rec_min = p->fasta ? (uint64_t)p->read_len[0] + 4 : 2 * (uint64_t)p->read_len[0] + 7;  // (">x", bases, two newlines)
    const uint64_t rows0 = reads_hint ? reads_hint + 16 : piece / rec_min + 16;
    rc = scalce_batch_create(ctx, p, rows0, cap + 256, &b);
    if (rc) { err = scalce_last_error(ctx); return rc; }
    scalce_batch_set_lean(b, (flags & SCALCE_STREAM_LEAN) ? 1 : 0);
    scalce_batch_set_keep_order(b, (flags & SCALCE_STREAM_KEEP_ORDER) ? 1 : 0);
    if ((flags & SCALCE_STREAM_KEEP_PLUS) && (rc = scalce_batch_set_keep_plus(b, 1))) { err = scalce_last_error(ctx); return rc; }
    if ((flags & SCALCE_STREAM_KEEP_COMMENTS) && (rc = scalce_batch_set_keep_comments(b, 1))) { err = scalce_last_error(ctx); return rc; }
    if ((flags & SCALCE_STREAM_KEEP_BASES) && (rc = scalce_batch_set_keep_bases(b, 1))) { err = scalce_last_error(ctx); return rc; }
  }
  const bool digest = (flags & SCALCE_STREAM_DIGEST) != 0;
  if (digest)
    for (int m = 0; m < nm; m++) {
      ST_HIP(dbuf_alloc(M[m].d_crc, sizeof(uint32_t) * Mate::CRC_SLOTS));
      ST_HIP(dbuf_alloc(M[m].d_crc_ws, scalce_crc32_ws_bytes(piece)));
      ST_HIP(M[m].h_crc.alloc(sizeof(uint32_t) * Mate::CRC_SLOTS));
      M[m].crc_ev.resize(Mate::CRC_SLOTS);
      for (Event &e : M[m].crc_ev) ST_HIP(e.create());
    }
  // the oldest open word of a mate joins its text's CRC; its event has long passed unless the ring is full or the run ends
  auto crc_join_oldest = [&](Mate &x) -> int {
    const std::pair<int, uint64_t> o = x.crc_open.front();
    if (hipEventSynchronize(x.crc_ev[o.first]) != hipSuccess) { err = "the digest of a chunk failed"; return SCALCE_ERR_HIP; }
    x.crc = scalce_crc32_combine(x.crc, x.h_crc.as<uint32_t>()[o.first], o.second);
    x.crc_open.pop_front();
    return SCALCE_OK;
  };
  // one launch over the chunk where it arrived, on the stream that takes it into the piece; the word follows it down
  auto crc_chunk = [&](Mate &x, int sl) -> int {
    int rc2;
    if ((int)x.crc_open.size() == Mate::CRC_SLOTS && (rc2 = crc_join_oldest(x))) return rc2;
    const int k = (int)(x.crc_chunks++ % Mate::CRC_SLOTS);
    if ((rc2 = scalce_crc32_device(ctx, x.d_raw[sl].as<uint8_t>(), x.raw_n[sl], x.d_crc.as<uint32_t>() + k, x.d_crc_ws.p, s_main))) { err = scalce_last_error(ctx); return rc2; }
    if (hipMemcpyAsync(x.h_crc.as<uint32_t>() + k, x.d_crc.as<uint32_t>() + k, sizeof(uint32_t), hipMemcpyDeviceToHost, s_main) != hipSuccess ||
        hipEventRecord(x.crc_ev[k], s_main) != hipSuccess) { err = "hipMemcpyAsync (chunk digest) failed"; return SCALCE_ERR_HIP; }
    x.crc_open.emplace_back(k, x.raw_n[sl]);
    return SCALCE_OK;
  };
  for (int m = 0; m < nm; m++) M[m].reader = std::thread(reader_main, &M[m].ring, rd[m], user[m], piece);

  // one more chunk of every mate that has input left and a free slot starts its way up
  auto upload = [&]() -> int {
    for (int m = 0; m < nm; m++) {
      Mate &x = M[m];
      if (x.eof || x.tail - x.head >= 2) continue;
      const int sl = (int)(x.tail & 1);
      ChunkRing::Chunk c;
      const double t0 = now_s();
      if (!x.ring.take_full(c)) { err = x.ring.error; return SCALCE_ERR_FORMAT; }
      S.read_wait_s += now_s() - t0;
      if (c.last) x.eof = true;
      x.raw_chunk[sl] = c;
      x.raw_n[sl] = c.n;
      // the slot's previous chunk must have left for d_text before this one lands on it
      if (x.landed_once[sl] && hipStreamWaitEvent(s_copy, x.land_ev[sl], 0) != hipSuccess) { err = "hipStreamWaitEvent failed"; return SCALCE_ERR_HIP; }
      if (c.n && hipMemcpyAsync(x.d_raw[sl].p, c.p, c.n, hipMemcpyHostToDevice, s_copy) != hipSuccess) { err = "hipMemcpyAsync (chunk upload) failed"; return SCALCE_ERR_HIP; }
      if (hipEventRecord(x.up_ev[sl], s_copy) != hipSuccess) { err = "hipEventRecord failed"; return SCALCE_ERR_HIP; }
      x.tail++;
      S.bytes[m] += c.n;
    }
    return SCALCE_OK;
  };
  // chunks that have arrived go behind the tail in d_text while the piece is short of `piece` bytes and they fit;
  // their pinned buffers return to the reader
  int landed = 0;
  auto land = [&]() -> int {
    landed = 0;
    for (int m = 0; m < nm; m++) {
      Mate &x = M[m];
      while (x.head < x.tail && x.have < piece && x.have + x.raw_n[x.head & 1] <= cap) {
        const int sl = (int)(x.head & 1);
        const double t0 = now_s();
        if (hipEventSynchronize(x.up_ev[sl]) != hipSuccess) { err = "chunk upload failed"; return SCALCE_ERR_HIP; }
        S.h2d_wait_s += now_s() - t0;
        if (digest && x.raw_n[sl]) { const int rc2 = crc_chunk(x, sl); if (rc2) return rc2; }
        if (x.raw_n[sl] && hipMemcpyAsync(x.text() + x.have, x.d_raw[sl].p, x.raw_n[sl], hipMemcpyDeviceToDevice, s_main) != hipSuccess) {
          err = "hipMemcpyAsync (piece assembly) failed";
          return SCALCE_ERR_HIP;
        }
        if (hipEventRecord(x.land_ev[sl], s_main) != hipSuccess) { err = "hipEventRecord failed"; return SCALCE_ERR_HIP; }
        x.landed_once[sl] = true;
        x.have += x.raw_n[sl];
        x.ring.put_free(x.raw_chunk[sl]);
        x.head++;
        landed++;
      }
    }
    return SCALCE_OK;
  };

  if ((rc = upload())) return rc;
  for (;;) {
    if ((rc = land())) return rc;
    if ((rc = upload())) return rc;  // travels while this piece is worked on
    bool final_piece = true;
    for (int m = 0; m < nm; m++) final_piece = final_piece && M[m].all_landed();
    uint64_t used[2] = {0, 0};
    const double t0 = now_s();
    rc = scalce_batch_append(b, M[0].text(), M[0].have, nm == 2 ? M[1].text() : nullptr, nm == 2 ? M[1].have : 0, final_piece ? 1 : 0, used, s_main);
    S.front_s += now_s() - t0;
    if (rc) { err = scalce_last_error(ctx); return rc; }
    S.rounds++;
    bool progress = landed > 0;
    for (int m = 0; m < nm; m++) {
      Mate &x = M[m];
      if (used[m] > x.have) { err = "internal: consumed more than the piece"; return SCALCE_ERR_ARG; }
      progress = progress || used[m] > 0;
      const uint64_t rest = x.have - used[m];
      if (rest && used[m]) {  // the unconsumed tail opens the next piece
        ST_HIP(hipMemcpyAsync(x.d_text[x.cur ^ 1].p, x.text() + used[m], rest, hipMemcpyDeviceToDevice, s_main));
        x.cur ^= 1;
      }
      x.have = rest;
    }
    if (final_piece) break;
    if (!progress) {
      err = "(ERROR) a record does not fit one piece of the stream (" + std::to_string(piece) + " bytes; a record of " +
            std::to_string(p->read_len[0]) + " bases is " + std::to_string(2 * (uint64_t)p->read_len[0] + 6) +
            " bytes and its name line), or the mates have different record counts";
      return SCALCE_ERR_FORMAT;
    }
  }
  double t0 = now_s();
  if ((rc = scalce_batch_order(b, s_main)) || (rc = scalce_batch_finish(b, s_main))) { err = scalce_last_error(ctx); return rc; }
  S.order_s = now_s() - t0;
  for (int m = 0; m < nm && digest; m++) {  // (the stream has just been waited for: every word is down)
    while (!M[m].crc_open.empty())
      if ((rc = crc_join_oldest(M[m]))) return rc;
    S.crc[m] = M[m].crc;
  }
  // the staging buffers are dead: give them back before the emit stage allocates the streams
  for (int m = 0; m < nm; m++)
    for (int i = 0; i < 2; i++) { M[m].d_text[i].release(); M[m].d_raw[i].release(); }
  t0 = now_s();
  if ((rc = scalce_batch_emit(b, s_main)) || (rc = scalce_batch_finish(b, s_main))) { err = scalce_last_error(ctx); return rc; }
  S.emit_s = now_s() - t0;
  if (!(flags & SCALCE_STREAM_DEFER_ENTROPY)) {
    t0 = now_s();
    if ((rc = scalce_batch_entropy(b, nullptr, s_main)) || (rc = scalce_batch_finish(b, s_main))) { err = scalce_last_error(ctx); return rc; }
    S.entropy_s = now_s() - t0;
  }
  return SCALCE_OK;
}

}  // namespace

extern "C" int scalce_stream_compress(scalce_ctx *ctx, const scalce_params *p, scalce_read_fn rd1, void *user1, scalce_read_fn rd2,
                                      void *user2, uint64_t piece_bytes, uint64_t reads_hint, int flags, scalce_batch **out,
                                      scalce_stream_stats *st, char *errbuf, size_t errcap) {
  if (!ctx || !p || !rd1 || !out || (p->paired && !p->interleaved && !rd2) || (p->interleaved && rd2)) return SCALCE_ERR_ARG;
  // streams read: one per mate, or ONE under -i (both mates in one text; scalce_batch_append takes whole pairs of it, so a
  // piece's tail that goes on into the next piece always begins at a pair)
  const int nm = p->paired && !p->interleaved ? 2 : 1;
  // a piece holds at least one record (-i: one pair) at its bound -- the fixed part, a name of up to 255 bytes, 32 to spare --,
  // or the tail of a piece could never grow into a whole record: reads of 2498 bases are 5 KB of text each
  uint64_t unit = 0;
  for (int m = 0; m < (p->paired ? 2 : 1); m++) unit += 2 * (uint64_t)(p->read_len[m] > 0 ? p->read_len[m] : 0) + 6 + 255 + 32;
  const uint64_t asked = piece_bytes ? piece_bytes : (1ull << 30);
  const uint64_t piece = ((asked > unit ? asked : unit) + 4095) & ~4095ull;
  scalce_read_fn rd[2] = {rd1, rd2};
  void *user[2] = {user1, user2};
  Stream s_copy, s_main;  // (in front of the mates: the streams go after the buffers and events used on them)
  Mate M[2];
  scalce_batch *b = nullptr;
  std::string err;
  scalce_stream_stats S;
  memset(&S, 0, sizeof S);
  const double t_start = now_s();
  const int rc = stream_run(ctx, p, rd, user, nm, piece, reads_hint, flags, s_copy, s_main, M, b, S, err);
  if (rc) {
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", err.c_str());
    if (b) scalce_batch_destroy(b);
    b = nullptr;
  } else {
    S.total_s = now_s() - t_start;
    S.reads = scalce_batch_reads(b);
  }
  // a reader blocked in rd() ends with its stream; one waiting for a free chunk is woken here.  Every reader is joined
  // before its pinned chunks go with the mates
  for (int m = 0; m < nm; m++) {
    M[m].ring.shutdown();
    if (M[m].reader.joinable()) M[m].reader.join();
  }
  if (st) *st = S;
  *out = b;
  return rc;
}
