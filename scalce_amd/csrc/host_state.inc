// host_state.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): context, core tables on the device, grow-only buffers, the shared workspace, the batch, read-backs
#include "hip_own.hpp"  // DBuf: the grow-only device buffer that frees itself

// the loaded table on the device (upload_tables): replaced as a whole by the next table
struct DeviceTables {
  DBuf d_next, d_outinfo, d_bucket_pattern, d_bucket_level;
  DBuf d_kmer;  // the k-mer block of the k-mer walks (null under the anchor walk, which does not read it)
  // anchor tables of tokenize_anchor_k, or null
  DBuf d_anchor_bits, d_anchor_rank, d_child_bits;
  DBuf d_anchor_single;  // per depth-K node: the ONE core below it (length, bucket, packed suffix), or 0 = walk
};
struct scalce_ctx : DeviceTables {
  int device = 0;
  std::string err;
  Automaton A;
  bool have_patterns = false;
  // what the table's walk reads (WalkTables, automaton.hpp): chosen and built when the table is loaded
  int walk = SCALCE_WALK_NONE;
  u32 id8_first = 0;
  DBuf d_simd_load;  // per (XCC, SE, SH, CU, SIMD): coder waves resident there (ac_encode_k's role choice)
  u32 anchor_K = 0, anchor_idK = 0;
};

static void set_err(scalce_ctx *c, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  c->err = buf;
}
// (for the other translation units of the library: sharded.cpp)
void scalce_set_last_error(scalce_ctx *c, const char *msg) { if (c) c->err = msg; }

#define HIP_TRY(ctx, expr)                                                               \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      set_err(ctx, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return SCALCE_ERR_HIP;                                                             \
    }                                                                                    \
  } while (0)

// A launch that the runtime refuses (a grid beyond 2^32 threads, say) must not pass for a kernel that ran: HIP's "last
// error" is overwritten by the next call that succeeds, so it is looked at right behind every launch and kept until
// scalce_batch_finish / the next read-back reports it.
static thread_local hipError_t g_launch_err = hipSuccess;
static thread_local const char *g_launch_what = "";
#define LAUNCH(kernel, grid, block, shmem, stream, ...)                                              \
  do {                                                                                               \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, stream, __VA_ARGS__);                 \
    const hipError_t le_ = hipGetLastError();                                                        \
    if (le_ != hipSuccess && g_launch_err == hipSuccess) { g_launch_err = le_; g_launch_what = #kernel; } \
  } while (0)
static int launch_failed(scalce_ctx *c) {
  if (g_launch_err == hipSuccess) return SCALCE_OK;
  set_err(c, "launch of %s failed: %s", g_launch_what, hipGetErrorString(g_launch_err));
  g_launch_err = hipSuccess;
  return SCALCE_ERR_HIP;
}
static inline u32 cdiv(u64 a, u64 b) {
  const u64 q = (a + b - 1) / b;
  return q > 0x7FFFFFFFull ? 0x7FFFFFFFu : (u32)q;  // callers whose grids can get there use grid-stride kernels
}

extern "C" int scalce_ctx_create(int device, scalce_ctx **out) {
  if (!out) return SCALCE_ERR_ARG;
  scalce_ctx *c = new scalce_ctx();
  c->device = device;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    // keep the context so the caller can read the message
    set_err(c, "no HIP device %d (found %d): this library has no CPU path", device, n);
    *out = c;
    return SCALCE_ERR_HIP;
  }
  if (hipSetDevice(device) != hipSuccess) {
    set_err(c, "hipSetDevice(%d) failed", device);
    *out = c;
    return SCALCE_ERR_HIP;
  }
  *out = c;
  HIP_TRY(c, hipMalloc(&c->d_simd_load.p, sizeof(u32) * AC_SIMD_KEYS));
  c->d_simd_load.cap = sizeof(u32) * AC_SIMD_KEYS;
  HIP_TRY(c, hipMemset(c->d_simd_load.p, 0, sizeof(u32) * AC_SIMD_KEYS));
  return SCALCE_OK;
}

static void free_tables(scalce_ctx *c) {
  static_cast<DeviceTables &>(*c) = DeviceTables();
  c->anchor_K = 0;
}

extern "C" void scalce_ctx_destroy(scalce_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);  // (the tables free themselves: on their device)
  delete c;
}
extern "C" const char *scalce_last_error(const scalce_ctx *c) { return c ? c->err.c_str() : "null context"; }

static int upload(scalce_ctx *c, DBuf &d, const void *src, size_t bytes) {
  d.release();
  HIP_TRY(c, hipMalloc(&d.p, bytes));
  d.cap = bytes;
  HIP_TRY(c, hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return SCALCE_OK;
}
#define UPLOAD(c, dptr, vec) do { int rc_ = upload(c, dptr, (vec).data(), sizeof((vec)[0]) * (vec).size()); if (rc_) return rc_; } while (0)
// the loaded table on the device: the DFA, the bucket tables and what its walk reads (build_walk_tables)
static int upload_tables(scalce_ctx *c) {
  free_tables(c);
  c->have_patterns = false;
  c->walk = SCALCE_WALK_NONE;
  const Automaton &A = c->A;
  WalkTables T;
  if (!build_walk_tables(A, T, c->err)) return SCALCE_ERR_FORMAT;
  HIP_TRY(c, hipSetDevice(c->device));
  UPLOAD(c, c->d_next, T.next);
  UPLOAD(c, c->d_outinfo, A.outinfo);
  UPLOAD(c, c->d_bucket_pattern, A.bucket_pattern);
  UPLOAD(c, c->d_bucket_level, A.bucket_level);
  c->id8_first = T.id8_first;
  if (T.walk == SCALCE_WALK_ANCHOR) {
    UPLOAD(c, c->d_anchor_single, T.anchor_single);
    UPLOAD(c, c->d_anchor_bits, T.anchor_bits);
    UPLOAD(c, c->d_anchor_rank, T.anchor_rank);
    UPLOAD(c, c->d_child_bits, T.child_bits);
    c->anchor_K = T.K;
    c->anchor_idK = T.idK;
  } else {
    UPLOAD(c, c->d_kmer, T.kmer);
  }
  c->walk = T.walk;
  c->have_patterns = true;
  return SCALCE_OK;
}

extern "C" int scalce_patterns_load_bin(scalce_ctx *c, const void *blob, size_t n) {
  if (!c || !blob) return SCALCE_ERR_ARG;
  if (!c->A.load_bin(blob, n)) { c->err = c->A.error; return SCALCE_ERR_FORMAT; }
  return upload_tables(c);
}
extern "C" int scalce_patterns_load_text(scalce_ctx *c, const char *text, size_t n) {
  if (!c || !text) return SCALCE_ERR_ARG;
  if (!c->A.load_text(text, n)) { c->err = c->A.error; return SCALCE_ERR_FORMAT; }
  return upload_tables(c);
}
extern "C" int scalce_patterns_count(const scalce_ctx *c) { return c ? (int)c->A.patterns.size() : 0; }
extern "C" int scalce_patterns_states(const scalce_ctx *c) { return c ? c->A.n_states : 0; }
extern "C" int scalce_patterns_buckets(const scalce_ctx *c) { return c ? c->A.n_buckets : 0; }
extern "C" int scalce_patterns_walk(const scalce_ctx *c, int *anchor_k) {
  if (anchor_k) *anchor_k = c ? (int)c->anchor_K : 0;
  return c ? c->walk : SCALCE_WALK_NONE;
}
extern "C" int scalce_pattern_length(const scalce_ctx *c, int p) {
  return (c && p >= 0 && p < (int)c->A.patterns.size()) ? (int)c->A.patterns[p].size() : -1;
}
extern "C" const char *scalce_pattern_string(const scalce_ctx *c, int p) {
  return (c && p >= 0 && p < (int)c->A.patterns.size()) ? c->A.patterns[p].c_str() : nullptr;
}

extern "C" int scalce_patterns_describe_host(const void *blob, size_t n, int is_text, int32_t *bucket_pattern_out,
                                            size_t cap, int32_t *n_states, int32_t *n_buckets) {
  // host-only view of the table builder (no device needed): emission order of the buckets
  Automaton A;
  const bool ok = is_text ? A.load_text(static_cast<const char *>(blob), n) : A.load_bin(blob, n);
  if (!ok) return SCALCE_ERR_FORMAT;
  if (n_states) *n_states = A.n_states;
  if (n_buckets) *n_buckets = A.n_buckets;
  if (bucket_pattern_out)
    for (size_t i = 0; i < cap && i < A.bucket_pattern.size(); i++) bucket_pattern_out[i] = A.bucket_pattern[i];
  return SCALCE_OK;
}

extern "C" int scalce_patterns_walk_host(const void *blob, size_t n, int is_text, int *anchor_k) {
  // the same without a device: what scalce_patterns_walk answers once the table is loaded
  Automaton A;
  WalkTables T;
  std::string err;
  if (anchor_k) *anchor_k = 0;
  if (!blob) return SCALCE_WALK_NONE;
  const bool ok = is_text ? A.load_text(static_cast<const char *>(blob), n) : A.load_bin(blob, n);
  if (!ok || !build_walk_tables(A, T, err)) return SCALCE_WALK_NONE;
  if (anchor_k) *anchor_k = (int)T.K;
  return T.walk;
}

extern "C" void scalce_params_default(scalce_params *p) {
  std::memset(p, 0, sizeof *p);
  p->use_names = 1;
  for (int m = 0; m < 2; m++) {
    p->qmap[m].offset = 33;
    for (int i = 0; i < 128; i++) p->qmap[m].values[i] = i;
    p->qprev[m][0] = p->qprev[m][1] = 500;
  }
  p->bucket_set_size = 0;
}

// ------------------------------------------------------------------------------------------------
enum { ST_INGEST = 0, ST_QUALITY, ST_TOKENIZE, ST_ORDER, ST_EMIT, ST_ENTROPY, ST_COUNT };

// Device buffers of the FRONT stages (ingest .. emit): rows, tokens, tie-break events, sort scratch.  Nothing behind the
// emit stage reads them -- the coder works on the reordered stream and writes the coded one -- so batches whose front stages
// run one after the other on one stream can share a single set (scalce_workspace): with six shards in flight that is the
// difference between 35 GB and 15 GB of HBM per shard (50 M reads x 100 bp).
// The rule: everything in here is valid for a batch only until another batch of the same workspace runs the stage that writes
// it; the *_owner fields mark the cases where a later stage checks.  (Stage code: `w.packed[m]` is the workspace's, `b->` the batch's.)
struct scalce_workspace {
  scalce_ctx *ctx = nullptr;
  u64 row_cap = 0;           // rows the run-wide arrays hold
  u64 piece_rows_cap = 0;    // records one piece may bring (size of the line index)
  DBuf line_end[2], tile[2], packed[2], q[2], namelen, namecell, outlen;
  DBuf names_in, name_in_off, prior_buf;  // names longer than a cell, input order
  DBuf tok_bucket, tok_pos, tie_index, tie_read, tie_off, tie_ncand, cand_bucket, cand_pos, choice;
  DBuf ev_off, ev_sorted, ev_tmp, ev_place, chosen, G, seg, dirty, cand_place, Gseg, cand_fixed;
  DBuf bucket, endv, tokens, counts, bucket_first, bucket_off, chunk, chunk_start;
  DBuf perm_a, perm_b, key_a, key_b, hist, scan_ws, S, run_head, run_hcount, run_rank, runid, run_items_a, run_items_b, run_pos;
  DBuf name_off;
  DBuf tw_cells, tw_cand, tw_bits, tw_base;  // the tie-break in windows (tokenize_windows)
  DBuf tile_mm[2];                           // per text tile: smallest / largest q' symbol (ingest_tiles2_k)
  const void *tile_mm_owner[2] = {nullptr, nullptr};  // the batch whose piece they describe (batches share a workspace)
  const void *walk_owner = nullptr;          // the batch whose first walk tok_bucket / tok_pos hold (scalce_batch_chunk_plan)
  DBuf cell_sorted;                          // name cells in output order (emit stage)
  DBuf qs_shared[2];                         // reordered q' stream of batches that only pass it on (scalce_batch_set_stream_scratch)
  DBuf alt_packed[2], alt_q[2], alt_namelen, alt_namecell, alt_name_in_off, alt_tok_bucket, alt_tok_pos;  // second set of row arrays (scalce_batch_rewindow)
  // Variable-length runs (params variable_length): padlen[m] = L - length per row, a run-wide row array beside namelen, 16 bits
  // per row; and the pad pass of the piece being ingested -- the line index of the caller's text, where each record begins in
  // the padded text (vl_off, one entry more: its size) and the padded text itself, which the ingest kernels then read
  DBuf padlen[2], vl_line_end[2], vl_off[2], vl_text[2];
  hipStream_t side = nullptr;                // the quality statistics beside the tie-break's sweeps (quality_beside): ONE more stream per workspace
  ~scalce_workspace() { if (side) hipStreamDestroy(side); }
};

// The counters of a batch that kernels write and the host reads back: ONE device allocation, a field per use, grouped by the
// stage that writes it.  The host only takes addresses in it (&b->d_scr->nev, b->d_scr->tri_tiles); nothing is cleared at
// creation, every stage presets what it needs.  What is cleared or read back together is one array or one struct (sizeof at
// the call site), and no field is lent from one stage to another: a new counter is a new field.
constexpr int SWEEPS_PER_LOOK = 4;  // global sweeps sent out per look at their flags (scalce_batch_tokenize_settle)
struct BatchScratch {
  // ---- ingest
  u64 nlines[2];         // newlines of a mate's text (piece_count)
  u64 consumed[2];       // per mate: text offset behind the last record taken (piece_unpack_t)
  u64 long_names_bytes;  // what the piece adds to the long-name store
  u64 text_offset;       // scalce_batch_text_offset
  u32 comment_longest[2];  // per mate: the run's longest entry (comment_plan_k; cleared when a run starts)
  u32 plus_longest[2];     // per mate: the run's longest stored '+'-line entry (plus_plan_k; cleared when a run starts)
  u32 plus_classes[2][2];  // per mate: repeated and literal entries of the run (plus_count_k at the emit stage)
  struct IngestFlags {   // cleared and read back as one
    u32 max_namelen;     // longest name of the piece
    u32 slow;            // a record did not fit the tile overlap: the piece is redone the indexed way
  } ingest;
  // ---- quality statistics (scalce_batch_quality).  Written on the workspace's SIDE stream while the tokenizer runs on the
  // main one (quality_beside): nothing in this group may be lent to the tokenizer, or to anything else that can run beside it.
  unsigned long long tri_tiles[TRI_MAX_PASSES];  // one tile counter per pass of trigram_pass_k
  struct TriCheck { u64 acc; u32 done, pad; } tri_check[2];  // tri_check_k, per mate: cleared as one
  u32 minmax[2];         // smallest / largest symbol of the piece
  u32 prev[2][2];        // per mate: the two symbols in front of the piece
  u32 range[2][3];       // per mate: {lo, A, all symbols inside}: span of the symbols that occur (scalce_batch_quality_plan reads it back)
  // ---- tokenize
  u64 cut_carry;         // bytes in the chunk left open behind the last cut (scalce_batch_chunk_plan)
  u32 ncuts;             // ... and how many cuts
  u32 ntie, ncand, nev, ntev;        // totals of the four scans that size the tie-break (scalce_batch_tokenize_begin)
  u32 sweep_moved[SWEEPS_PER_LOOK];  // per global sweep: a decision moved
  // ---- order
  u32 nchunks;           // spill chunks (chunk_bounds_k or the caller's; chunk_assign_k reads it)
  u32 run_members;       // records in the runs that phase 2 sorts
  u32 any_large;         // a run too long for run_small_sort_k
  // ---- emit
  struct EmitTotals { u64 reads, read_bytes, name_bytes; } emit;  // totals of its three scans, read back in one go
  // ---- entropy
  u64 frame_bytes[2];    // per mate: the framed stream (ac_frame, entropy_windowed)
  struct TableInfo {     // per mate, ac_table_k: cleared and read back as one
    u64 max_total;       // largest context total (a u32 atomicMax on the low word)
    unsigned long long cost[2];  // the table's own coding cost in 1/256 bit, and the symbols it counts
  } tinfo[2];
};

struct scalce_batch {
  scalce_workspace *ws;  // front-stage buffers: the batch's own, or shared with other batches (scalce_batch_create_shared)
  bool owns_ws;
  scalce_batch(scalce_workspace *w, bool owns) : ws(w), owns_ws(owns) {}
  ~scalce_batch();
  scalce_ctx *ctx = nullptr;
  scalce_params p;
  u64 max_reads = 0, max_text = 0;
  int nm = 1;
  int L[2] = {0, 0}, stride[2] = {0, 0}, szr[2] = {0, 0}, sz_meta = 1;
  // Records without qualities (params fasta / no_qualities): lpr = text lines per record (2 under fasta, else 4); nq = no q'
  // anywhere -- no q' rows, no quality statistics, no table, no coder, and the -B rule counts no quality bytes.
  int lpr = 4;
  bool nq = false;
  // Interleaved pairs (params interleaved, -i): nm = 2, but ONE text per piece -- record 2k + m of it is mate m of row k.  The
  // piece's newline counts and line index are mate 0's (tile[0], line_end[0]) and serve both mates; ntext = texts per piece.
  bool il = false;
  int ntext = 1;
  bool vl = false;  // reads of different lengths (params variable_length): a pad pass in front of the ingest (pad_piece)
  int vl_mate = 0;  // ... and the mate whose piece it padded last (which read length an error speaks of)
  u64 unit_lines() const { return (u64)lpr * (il ? 2 : 1); }  // text lines per row: a record, or a pair
  // Rows.  A batch takes its input in one piece (scalce_batch_ingest) or in several (scalce_batch_append): rows
  // [base, base + NP) are the piece being ingested / tokenized, N = base + NP is everything the batch holds.  Packed
  // bases, q', names and tokens are run-wide arrays indexed by row; the text of a piece is dead once it is ingested.
  u64 N = 0, base = 0, NP = 0;
  u64 tok_done = 0, tok_base = 0, tok_n = 0;  // rows tokenized so far / the rows of the tokenization in progress
  bool appending = false;    // the pieces came through scalce_batch_append
  bool lean = false;         // release what a stage no longer needs (runs sized for most of HBM)
  bool keep_order = false;   // SCALCE_OUT_PERM is an output of the run: a lean batch keeps it (scalce_batch_set_keep_order)
  u64 tri_expected[2] = {0, 0};  // trigrams counted so far (tri_check_k)
  u32 quality_source[2] = {0, 0};  // where the last scalce_batch_quality took the mate's symbol range from (scalce_batch_quality_plan)
  u32 ingest_plan[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // what the last piece_unpack_t did for the mate (scalce_batch_ingest_plan)
  u64 names_in_used = 0;     // bytes of the long-name store in use
  u64 S_rows = ~0ull;        // rows the record-size prefix sums in S cover (scalce_batch_chunk_plan), ~0 = stale
  u64 walk_rows = 0;         // rows [0, walk_rows) whose first tokenizer walk (tok_bucket / tok_pos) scalce_batch_chunk_plan has
                             // already done: scalce_batch_tokenize_begin over exactly these rows does not walk them again
  u64 text_bytes[2] = {0, 0};
  const u8 *piece_text[2] = {nullptr, nullptr};  // the piece ingested last (its line index is built on demand)
  bool line_index_ok[2] = {false, false};
  u64 piece_consumed[2] = {0, 0};               // text offset behind the last record taken from it
  bool ingested[2] = {false, false};
  // device state
  DevErr *d_err = nullptr;
  BatchScratch *d_scr = nullptr;  // the counters the stages read back (device memory: the host only takes addresses in it)
  u32 *h_pub = nullptr, *h_pub_dev = nullptr;  // a page of fine-grained host memory the read-backs are published into (read_words)
  u32 pub_seq = 0;
  u8 *d_qlut[2] = {nullptr, nullptr};
  int q_affine[2] = {-1, -1};  // the quality map is q - offset for every character: no table lookups in the ingest kernel
  // what the coder and the caller read behind the emit stage: the batch's own
  DBuf freq4[2], table[2], qs_own[2], counts_total, bucket_name_bytes, ac_scan;
  // The reordered q' stream: the batch's own (the coder reads it long after the emit stage), or -- scalce_batch_set_stream_scratch,
  // sharded runs: the stream is handed to other ranks right behind the emit stage and the coder reads what came back -- the
  // workspace's, valid until the next batch of the workspace runs its emit stage.
  bool qs_in_ws = false;
  DBuf &qs(int m) { return qs_in_ws ? ws->qs_shared[m] : qs_own[m]; }
  const DBuf &qs(int m) const { return qs_in_ws ? ws->qs_shared[m] : qs_own[m]; }
  const u64 *sorted_keys = nullptr;  // phase-1 keys in output order (order stage), consumed by the emit stage
  u32 key_end_bits = 0, key_bucket_shift = 0, key_bucket_mask = 0;
  bool mm_valid[2] = {false, false};  // the workspace's tile_mm[m] holds the symbol ranges of the piece ingested last
  bool names_from_sorted_cells = false;
  u32 order_run_members = 0;
  u32 order_radix_fallback = 0;  // any_large as read back: phase 2 went through the radix passes (0: it did not, or did not run)
  DBuf out_reads[2], out_names, ac_tab[2], ac_tab8[2], ac_cum[2], ac_blocks[2], ac_sizes[2], ac_off[2], ac_desc, out_qual[2];
  AcBlockDesc *ac_desc_host = nullptr;  // block descriptors of the last coder launch this shard led: pinned, so that the
  u32 ac_desc_cap = 0;                  // asynchronous upload never reads memory the next launch is already rewriting
  u32 *perm = nullptr;  // final permutation (points into perm_a or perm_b)
  DBuf out_lengths[2];  // variable-length runs: L - length in output order (the order stage gathers padlen through perm)
  // What follows the names (scalce_batch_set_keep_comments): per mate comlen = the entry's length per row (u16, run-wide, input
  // order) and com_in = the entries, each with its newline, in input order (com_used bytes of it, like the long-name store);
  // the emit stage gathers them through the permutation into out_comments (SCALCE_OUT_COMMENTS).  com_off / com_out_off /
  // com_piece_off: the offsets of the gather and of a piece's extract pass.  Nothing of it exists without the option.
  bool keep_comments = false;
  DBuf comlen[2], com_in[2], out_comments[2], com_off, com_out_off, com_piece_off, com_ws;
  u64 com_used[2] = {0, 0}, out_comments_bytes[2] = {0, 0};
  u32 com_longest[2] = {0, 0};
  // The '+' lines (scalce_batch_set_keep_plus): the same shape once more -- pluslen = the stored entry's length per row (0 bare,
  // 1 repeat, 1 + bytes literal), plus_in the entries with class byte and newline in input order, out_plus what the emit stage
  // gathers (SCALCE_OUT_PLUS).  The offsets and the scratch of the gather are the comments' when both are on, since the
  // gathers run one behind the other.  Nothing of it exists without the option.
  bool keep_plus = false;
  DBuf pluslen[2], plus_in[2], out_plus[2];
  u64 plus_used[2] = {0, 0}, out_plus_bytes[2] = {0, 0};
  u32 plus_longest[2] = {0, 0}, plus_repeats[2] = {0, 0}, plus_literals[2] = {0, 0};
  // The letters and qualities the archive does not keep (scalce_batch_set_keep_bases): per mate exc_cnt = the exceptions per
  // row (u16, run-wide, input order) and exc_in = their entries in input order (exc_used of them); the emit stage gathers
  // them through the permutation into out_exc (SCALCE_OUT_EXCEPTIONS) with the archive index stamped in.  exc_piece_off /
  // exc_off / exc_out_off: the offsets of a piece's write pass and of the gather.  Nothing of it exists without the option.
  bool keep_bases = false;
  DBuf exc_cnt[2], exc_in[2], out_exc[2], exc_piece_off, exc_off, exc_out_off, exc_ws;
  u64 exc_used[2] = {0, 0}, exc_rows[2] = {0, 0}, out_exc_entries[2] = {0, 0};
  // host-side results
  u64 out_reads_bytes[2] = {0, 0}, out_names_bytes = 0, out_qual_bytes[2] = {0, 0};
  u32 ntie = 0, nev = 0, ntev = 0, ncand_cap = 0, jacobi_iters = 0, nchunks = 1, sweep_no = 0;
  bool tie_fallback = false;  // the last tie-break ended in tie_sequential_k
  u32 tie_plan[4] = {0, 0, 0, 0};  // path, tie reads per window, windows, counters of tie_sequential_k (scalce_batch_tie_plan)
  bool tok_open = false;
  int dirty_cur = 0;
  std::vector<uint64_t> explicit_chunks;  // spill-chunk starts given by the caller (sharded runs), else -B rule
  // stage timing
  bool timing = false;
  float stage_ms[ST_COUNT] = {0};
  int stage_launches[ST_COUNT] = {0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_group = nullptr;
  // the quality statistics beside the tie-break's sweeps (scalce_batch_front, quality_beside) on the workspace's side stream
  hipEvent_t ev_fork = nullptr, ev_side = nullptr;
  bool quality_deferred = false, side_busy = false;
  u32 tri_grid = 256;  // workgroups of trigram_pass_k (one per CU)
  // HIP-event pairs around every ac_encode_k launch (the dominant kernel); read by scalce_batch_kernel_ms
  int ac_round_launched = 0;  // symbols per round of the last ac_encode_lanes_k launch this batch led (0: none yet)
  bool ktiming = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
  size_t kev_used = 0;
  u64 k_in_bytes = 0, k_out_bytes = 0;
  // entropy launched but its result size not read back yet (scalce_batch_entropy_begin / _end): blocks per mate
  u32 ent_pending[2] = {0, 0};
  u32 frame_deferred[2] = {0, 0};  // blocks coded by a grouped launch and not framed yet (entropy_collect frames them)
  // Framing on demand (scalce_batch_set_frame_on_demand): the coded blocks stay where the coder wrote them; entropy_collect
  // only lays the frames out (ac_off: where block k's [u32 size][bytes] begins in the stream).  The stream itself is
  // produced on its way out -- scalce_batch_qual_window, into device or pinned host memory -- or, for callers that ask for
  // SCALCE_OUT_QUAL as a device pointer, once, at that moment.
  // Bytes per block of the coder's output buffers.  The reference gives every block 10 MiB (arithmetic.cpp:301); sized like that
  // a 50 M-read shard holds 5 GB of which 2.9 are used.  ac_prepare sizes the stride from what the table says coding its own
  // counts costs (+ 8 % + 64 KiB); a block that outgrows it reports E_ACOVERFLOW and the shard is coded again at the full
  // stride when it is collected (entropy_recode_full) -- same bytes, one launch later.
  // One row per read (single-end runs, read lengths the tile ingest takes): q[0] holds rows of `qstride[0]` bytes -- q' | a copy
  // of the packed words: 128 bytes = one aligned line for a 100 bp read -- and the emit stage gathers a record's q' and bases
  // with ONE random line (emit_reads_k<true>).  Otherwise qstride[m] = L[m]: rows back to back.
  bool fused = false;
  u32 qstride[2] = {0, 0}, row_cell_off = 0, row_pwords = 0;
  DBuf q_compact, fuse_q;  // SCALCE_OUT_QINPUT of fused rows on request; classic arrays of a piece the indexed kernels took
  u64 ac_stride[2] = {0, 0};
  // Coding in place (scalce_batch_set_code_in_place): the coder's output goes over the symbols it has consumed -- block k's bytes
  // begin where block k's symbols began, ac_base = the reordered stream itself, ac_stride = 10 MiB -- and the batch holds no
  // block buffers at all (3.2 GB per 50 M reads of 100 bp).  A block whose output would catch up with its input reports
  // E_ACOVERFLOW; its symbols are gone by then, so the shard is run again FROM ITS TEXT with buffers of its own
  // (entropy_rerun_from_text: the caller keeps the text of a shard in place until the shard is collected).
  bool code_in_place = false, in_place_suspended = false;
  u64 reruns = 0;                          // shards run again from their text (entropy_rerun_from_text)
  bool in_place_now[2] = {false, false};   // the last launch coded this mate's stream in place
  u8 *ac_base[2] = {nullptr, nullptr};     // block k of the last launch: ac_base + k * ac_stride
  DBuf ac_log[2];                          // carry notes of ac_encode_lanes_k when the block's buffer has no room for them
  const u8 *ac_last_sym[2] = {nullptr, nullptr};  // what the last launch coded (for the recode)
  u64 ac_last_nsym[2] = {0, 0};
  bool frame_on_demand = false;
  u32 frame_virtual[2] = {0, 0};   // blocks whose frames are laid out but not copied (0: out_qual holds the stream)
  std::vector<u64> frame_off_host[2];  // where block k's frame begins (host copy, taken when the stage is collected)
  // symbol stream to code per mate: the shard's own reordered stream, or one the caller assembled (sharded runs)
  const u8 *ent_sym[2] = {nullptr, nullptr};
  u64 ent_nsym[2] = {0, 0};
  bool ent_external[2] = {false, false};
};

static int ensure(scalce_batch *b, DBuf &d, size_t bytes) {
  if (bytes <= d.cap) return SCALCE_OK;
  // (an allocation synchronises the whole device: in a pipeline it waits for every coder that is running.  SCALCE_TRACE=1
  //  names the ones that still happen after the warm-up)
  static const bool dbg = getenv("SCALCE_TRACE") != nullptr;
  if (dbg) fprintf(stderr, "scalce: batch %p grows a buffer from %zu to %zu bytes\n", (void *)b, d.cap, bytes);
  d.release();
  bytes = (bytes + 255) & ~size_t(255);
  hipError_t e = hipMalloc(&d.p, bytes);
  if (e != hipSuccess) {
    set_err(b->ctx, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return SCALCE_ERR_HIP;
  }
  d.cap = bytes;
  return SCALCE_OK;
}
#define ENSURE(b, buf, bytes) do { int rc_ = ensure(b, buf, bytes); if (rc_) return rc_; } while (0)
// the same for run-wide arrays that grow while a run is ingested piece by piece: the first `used` bytes survive
static int ensure_keep(scalce_batch *b, DBuf &d, size_t bytes, size_t used, hipStream_t s) {
  if (bytes <= d.cap) return SCALCE_OK;
  if (!d.p || !used) return ensure(b, d, bytes);
  size_t want = d.cap + d.cap / 2;
  if (want < bytes) want = bytes;
  want = (want + 255) & ~size_t(255);
  void *np = nullptr;
  hipError_t e = hipMalloc(&np, want);
  if (e != hipSuccess && want > bytes) { want = (bytes + 255) & ~size_t(255); e = hipMalloc(&np, want); }
  if (e != hipSuccess) {
    set_err(b->ctx, "hipMalloc(%zu) failed while growing a run-wide array: %s", want, hipGetErrorString(e));
    return SCALCE_ERR_HIP;
  }
  if ((e = hipMemcpyAsync(np, d.p, used, hipMemcpyDeviceToDevice, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) {
    hipFree(np);
    set_err(b->ctx, "growing a run-wide array: %s", hipGetErrorString(e));
    return SCALCE_ERR_HIP;
  }
  hipFree(d.p);
  d.p = np;
  d.cap = want;
  return SCALCE_OK;
}
scalce_batch::~scalce_batch() {  // (the DBufs free themselves)
  if (owns_ws) delete ws;
  if (d_err) hipFree(d_err);
  if (d_scr) hipFree(d_scr);
  if (h_pub) hipHostFree(h_pub);
  for (int m = 0; m < 2; m++) if (d_qlut[m]) hipFree(d_qlut[m]);
  if (ac_desc_host) hipHostFree(ac_desc_host);
  for (hipEvent_t e : {ev_fork, ev_side, ev0, ev1, ev_group}) if (e) hipEventDestroy(e);
  for (auto &pr : kev) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
}

static inline int sz_read(int l) { return (l + 3) / 4; }
// room behind the reordered stream: the last block of a stream coded in place may write this much more than it holds symbols
constexpr size_t AC_INPLACE_PAD = 65536;

// run-wide arrays indexed by row: room for `rows` of them, the first `used` rows kept
static int reserve_rows(scalce_batch *b, u64 rows, u64 used, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  if (rows <= w.row_cap) return SCALCE_OK;
  if (rows >= (1ull << 32) - 64) { set_err(b->ctx, "a batch holds fewer than 2^32 reads"); return SCALCE_ERR_CAPACITY; }
  if (w.row_cap && rows < w.row_cap + w.row_cap / 4) rows = w.row_cap + w.row_cap / 4;  // grow in steps
  int rc;
  for (int m = 0; m < b->nm; m++) {
    if ((rc = ensure_keep(b, w.packed[m], (size_t)b->stride[m] * rows + 64, (size_t)b->stride[m] * used, s))) return rc;
    if (!b->nq && (rc = ensure_keep(b, w.q[m], (size_t)b->qstride[m] * rows + 64, (size_t)b->qstride[m] * used, s))) return rc;
  }
  if ((rc = ensure_keep(b, w.namelen, rows + 64, used, s))) return rc;
  for (int m = 0; m < b->nm && b->vl; m++)
    if ((rc = ensure_keep(b, w.padlen[m], sizeof(u16) * (rows + 64), sizeof(u16) * used, s))) return rc;
  if (b->p.use_names && (rc = ensure_keep(b, w.namecell, 16 * (rows + 8), 16 * used, s))) return rc;
  if (w.name_in_off.p && (rc = ensure_keep(b, w.name_in_off, sizeof(u64) * (rows + 2), sizeof(u64) * used, s))) return rc;
  if ((rc = ensure_keep(b, w.bucket, sizeof(u32) * (rows + 1), sizeof(u32) * used, s))) return rc;
  if ((rc = ensure_keep(b, w.endv, sizeof(u16) * (rows + 1), sizeof(u16) * used, s))) return rc;
  if ((rc = ensure_keep(b, w.tokens, sizeof(int32_t) * 2 * (rows + 1), sizeof(int32_t) * 2 * used, s))) return rc;
  w.row_cap = rows;
  return SCALCE_OK;
}

extern "C" int scalce_workspace_create(scalce_ctx *c, scalce_workspace **out) {
  if (!c || !out) return SCALCE_ERR_ARG;
  *out = new scalce_workspace();
  (*out)->ctx = c;
  return SCALCE_OK;
}
extern "C" void scalce_workspace_destroy(scalce_workspace *w) {
  if (!w) return;
  hipSetDevice(w->ctx->device);  // (in front of every delete: the buffers free themselves on the current device)
  delete w;
}

static int batch_create(scalce_ctx *c, const scalce_params *p, uint64_t max_reads, uint64_t max_text, scalce_workspace *shared,
                        scalce_batch **out);
extern "C" int scalce_batch_create(scalce_ctx *c, const scalce_params *p, uint64_t max_reads, uint64_t max_text,
                                   scalce_batch **out) {
  return batch_create(c, p, max_reads, max_text, nullptr, out);
}
extern "C" int scalce_batch_create_shared(scalce_ctx *c, const scalce_params *p, uint64_t max_reads, uint64_t max_text,
                                          scalce_workspace *w, scalce_batch **out) {
  if (!w || w->ctx != c) return SCALCE_ERR_ARG;
  return batch_create(c, p, max_reads, max_text, w, out);
}
static int batch_create(scalce_ctx *c, const scalce_params *p, uint64_t max_reads, uint64_t max_text, scalce_workspace *shared,
                        scalce_batch **out) {
  if (!c || !p || !out) return SCALCE_ERR_ARG;
  if (!c->have_patterns) { set_err(c, "load a core table first"); return SCALCE_ERR_ARG; }
  if (p->interleaved && !p->paired) { set_err(c, "interleaved input (-i) is paired: set paired as well"); return SCALCE_ERR_ARG; }
  if (p->read_len[0] <= 0 || p->read_len[0] > 2498 || (p->paired && (p->read_len[1] <= 0 || p->read_len[1] > 2498))) {
    set_err(c, "read_len must be set (1..2498: the reference reads lines into MAXLINE = 2500 bytes, const.h:87)");
    return SCALCE_ERR_ARG;
  }
  if (max_reads >= (1ull << 32) - 64) { set_err(c, "a shard holds fewer than 2^32 reads"); return SCALCE_ERR_CAPACITY; }
  if (p->variable_length && (p->fasta || p->no_qualities || p->interleaved)) {
    set_err(c, "variable-length reads (--variable-length) are not available together with %s",
            p->fasta ? "FASTA input (-f)" : p->no_qualities ? "dropped qualities (-Q)" : "interleaved input (-i)");
    return SCALCE_ERR_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  scalce_workspace *w = shared;
  if (!w) { w = new scalce_workspace(); w->ctx = c; }
  scalce_batch *b = new scalce_batch(w, shared == nullptr);
  b->ctx = c;
  b->p = *p;
  b->max_reads = max_reads;
  b->max_text = max_text;
  b->nm = p->paired ? 2 : 1;
  b->il = p->interleaved != 0;
  b->ntext = b->il ? 1 : b->nm;
  b->vl = p->variable_length != 0;
  for (int m = 0; m < b->nm; m++) {
    b->L[m] = p->read_len[m];
    b->szr[m] = sz_read(b->L[m]);
    b->stride[m] = ((b->szr[m] + 1 + 15) / 16) * 16;  // one spare zero byte for 16-bit digit windows
  }
  b->sz_meta = b->L[0] > 255 ? 2 : 1;  // reads.cpp:106-108
  b->lpr = p->fasta ? 2 : 4;
  b->nq = p->fasta || p->no_qualities;
  b->qstride[0] = b->nq ? 0u : (u32)b->L[0];
  b->qstride[1] = b->nq ? 0u : (u32)b->L[1];
  if (b->nm == 1 && !b->nq && (b->L[0] & 3) == 0 && b->L[0] >= 16 && b->L[0] <= 160) {
    b->fused = true;
    b->row_cell_off = (u32)b->L[0];   // where the packed words begin
    b->row_pwords = (u32)(b->L[0] + 15) / 16;
    b->qstride[0] = (b->row_cell_off + 4 * b->row_pwords + 15) / 16 * 16;
  }
  *out = b;
  HIP_TRY(c, hipMalloc(&b->d_err, sizeof(DevErr)));
  HIP_TRY(c, hipMemset(b->d_err, 0, sizeof(DevErr)));
  HIP_TRY(c, hipMalloc(&b->d_scr, sizeof(BatchScratch)));
  if (hipHostMalloc(reinterpret_cast<void **>(&b->h_pub), 4096, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable) == hipSuccess) {
    memset(b->h_pub, 0, 4096);
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_pub_dev), b->h_pub, 0) != hipSuccess) { hipHostFree(b->h_pub); b->h_pub = nullptr; }
  } else {
    b->h_pub = nullptr;  // (read-backs then go through hipMemcpyAsync)
    (void)hipGetLastError();
  }
  HIP_TRY(c, hipEventCreate(&b->ev0));
  HIP_TRY(c, hipEventCreate(&b->ev1));
  for (int m = 0; m < b->nm && !b->nq; m++) {  // (nothing of the quality model without qualities)
    u8 lut[128];
    bool identity = p->qmap[m].offset >= 0 && p->qmap[m].offset < 128;
    for (int i = 0; i < 128; i++) {
      lut[i] = (u8)((p->qmap[m].values[i] - p->qmap[m].offset) & 255);
      identity = identity && p->qmap[m].values[i] == i;
    }
    b->q_affine[m] = identity ? (int)p->qmap[m].offset : -1;
    HIP_TRY(c, hipMalloc(&b->d_qlut[m], 128));
    HIP_TRY(c, hipMemcpy(b->d_qlut[m], lut, 128, hipMemcpyHostToDevice));
    ENSURE(b, b->freq4[m], sizeof(u64) * 512000);
    ENSURE(b, b->table[m], sizeof(u32) * 512000);
  }
  // a record is at least "@x", L bases, "+", L qualities and four newlines (">x", L bases and two newlines under -f): what
  // one piece of max_text bytes can bring
  const u64 per_piece = max_text / (b->lpr == 2 ? (u64)b->L[0] + 4 : 2 * (u64)b->L[0] + 7) + 2;
  w->piece_rows_cap = per_piece < max_reads ? per_piece : max_reads;
  // (the line index of a piece, 32 bytes per record, is only built when something asks for it: ensure_line_index)
  { int rc = reserve_rows(b, max_reads, 0, nullptr); if (rc) return rc; }
  ENSURE(b, w->scan_ws, sizeof(u64) * (scan_ws_elems(4 * w->piece_rows_cap + 1024) + 4096));
  return SCALCE_OK;
}

extern "C" void scalce_batch_destroy(scalce_batch *b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  delete b;
}

struct StageTimer {
  scalce_batch *b;
  int st;
  hipStream_t s;
  StageTimer(scalce_batch *b_, int st_, hipStream_t s_) : b(b_), st(st_), s(s_) {
    if (b->timing) hipEventRecord(b->ev0, s);
  }
  ~StageTimer() {
    if (b->timing) {
      hipEventRecord(b->ev1, s);
      hipEventSynchronize(b->ev1);
      float ms = 0;
      hipEventElapsedTime(&ms, b->ev0, b->ev1);
      b->stage_ms[st] += ms;
      b->stage_launches[st]++;
    }
  }
};

// ---- read-backs ----------------------------------------------------------------------------------------------
// A few counters per stage size the next launches: ~34 read-backs per shard.  As hipMemcpyAsync into pageable memory +
// hipStreamSynchronize each left the stream idle for ~40 us (a blit kernel, then the runtime's wake-up): 1.4 ms of a shard's
// 36 when nothing else runs beside its front stages.  Here a one-wave kernel copies the words into a page of fine-grained host
// memory and stores a sequence number behind them (system scope); the host spins on that word.  When the stream has drained
// and the number has not come (a launch the runtime refused), or when the page could not be had: the old way.
constexpr u32 PUB_WORDS = 960;
__global__ __launch_bounds__(64) void publish_k(const u32 *src, u32 nwords, u32 *page, u32 seq) {
  for (u32 k = threadIdx.x; k < nwords; k += 64) page[16 + k] = src[k];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(&page[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static int read_words(scalce_batch *b, const void *d, void *h, u32 nwords, hipStream_t s) {
  { int rc = launch_failed(b->ctx); if (rc) return rc; }
  if (b->h_pub && nwords <= PUB_WORDS) {
    u32 seq = ++b->pub_seq;
    if (!seq) seq = ++b->pub_seq;
    hipLaunchKernelGGL(publish_k, dim3(1), dim3(64), 0, s, static_cast<const u32 *>(d), nwords, b->h_pub_dev, seq);
    if (hipGetLastError() == hipSuccess) {
      for (u64 spins = 1;; spins++) {
        if (__atomic_load_n(&b->h_pub[0], __ATOMIC_ACQUIRE) == seq) { memcpy(h, b->h_pub + 16, sizeof(u32) * nwords); return SCALCE_OK; }
        if ((spins & 0x3FFF) == 0) {  // now and then: is the stream still at work at all?
          const hipError_t q = hipStreamQuery(s);
          if (q == hipSuccess) {
            if (__atomic_load_n(&b->h_pub[0], __ATOMIC_ACQUIRE) == seq) { memcpy(h, b->h_pub + 16, sizeof(u32) * nwords); return SCALCE_OK; }
            break;  // drained without publishing: fall through to the copy, which reports what happened
          }
          if (q != hipErrorNotReady) { set_err(b->ctx, "hipStreamQuery: %s", hipGetErrorString(q)); return SCALCE_ERR_HIP; }
        }
        __builtin_ia32_pause();
      }
    }
  }
  HIP_TRY(b->ctx, hipMemcpyAsync(h, d, sizeof(u32) * nwords, hipMemcpyDeviceToHost, s));
  HIP_TRY(b->ctx, hipStreamSynchronize(s));
  return SCALCE_OK;
}
static int read_u32(scalce_batch *b, const u32 *d, u32 *h, int n, hipStream_t s) { return read_words(b, d, h, (u32)n, s); }
static int read_u64(scalce_batch *b, const u64 *d, u64 *h, int n, hipStream_t s) { return read_words(b, d, h, 2u * (u32)n, s); }

static int check_device_error(scalce_batch *b, hipStream_t s) {
  { int rc = launch_failed(b->ctx); if (rc) return rc; }
  DevErr e;
  { int rc = read_words(b, b->d_err, &e, (u32)(sizeof e / 4), s); if (rc) return rc; }
  if (e.code == E_NONE) return SCALCE_OK;
  static const char *names[] = {"", "line count is not a multiple of 4 or the text does not end in a newline",
                                "read or quality line length differs from read_length (compress.cpp:628-634)",
                                "read name longer than 255 bytes or empty name line",
                                "quality symbol >= 80 after mapping (arithmetic.h:47)",
                                "arithmetic-coded block larger than the reference's 10 MiB buffer (arithmetic.cpp:101)",
                                "mates have different record counts", "internal"};
  if (b->vl && e.code == E_READLEN)
    set_err(b->ctx, "(ERROR) record %llu holds %u bases, more than the run's read length (%d%s): give the longest read with --max-length",
            (unsigned long long)e.where, e.aux, b->L[b->vl_mate], b->nm == 2 ? (b->vl_mate ? ", mate 2" : ", mate 1") : "");
  else if (e.code == E_COMMENT)
    set_err(b->ctx, "(ERROR) record %llu: what follows the name is longer than 65535 bytes", (unsigned long long)e.where);
  else if (e.code == E_PLUSLINE)
    set_err(b->ctx, "(ERROR) record %llu: the third line does not begin with '+'", (unsigned long long)e.where);
  else if (e.code == E_PLUSLONG)
    set_err(b->ctx, "(ERROR) record %llu: the '+' line is longer than 65535 bytes", (unsigned long long)e.where);
  else if (e.code == E_SEQQUAL)
    set_err(b->ctx, "(ERROR) record %llu: its sequence line (%u characters) and its quality line differ in length", (unsigned long long)e.where, e.aux);
  else
    set_err(b->ctx, "(ERROR) %s [record/block %llu, aux %u]", names[e.code < 8 ? e.code : 7], (unsigned long long)e.where, e.aux);
  hipMemsetAsync(b->d_err, 0, sizeof(DevErr), s);
  return SCALCE_ERR_FORMAT;
}
