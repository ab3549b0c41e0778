// host_tokenize.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): stage 2: both walks, events, the exact tie-break (windows, global sweeps, sequential bound), spill-chunk plan
// the anchor walk's view of the table and of `nrec` rows from `packed` on (tokenize_anchor_k; the candidate pass adds its own)
static void anchor_args(const scalce_ctx *c, const scalce_batch *b, const u8 *packed, u64 nrec, AnchorArgs &a) {
  memset(&a, 0, sizeof a);
  a.next = c->d_next.as<u32>(); a.outinfo = c->d_outinfo.as<u32>();
  a.bits = c->d_anchor_bits.as<u64>(); a.rank = c->d_anchor_rank.as<u32>(); a.child = c->d_child_bits.as<u32>(); a.K = c->anchor_K; a.idK = c->anchor_idK;
  a.single = c->d_anchor_single.as<uint4>();
  a.packed = packed; a.nrec = nrec; a.L = b->L[0]; a.stride = b->stride[0]; a.root_bucket = (u32)c->A.n_buckets;
}
// The one place a tokenizer walk is launched: the walk the loaded table selected (scalce_ctx::walk) over rows
// [row0, row0 + n), whose tokens live in tok_bucket / tok_pos at index (row - tok_row0).
//   WALK_FIRST       every row: longest core, its last base, hits at that length, tie flag -> tok_bucket / tok_pos
//   WALK_CANDIDATES  the b->ntie tie reads among them (tie_read counts from row0): the distinct cores of the longest length
//                    in order of first appearance -> cand_bucket / cand_pos / tie_ncand
static void launch_walk(scalce_batch *b, WalkPass pass, u64 row0, u64 n, u64 tok_row0, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  const scalce_ctx *c = b->ctx;
  const bool cands = pass == WALK_CANDIDATES, t7 = c->walk == SCALCE_WALK_KMER_T7;
  const u32 ntie = cands ? b->ntie : 0;
  if (!(cands ? (u64)ntie : n)) return;
  const u8 *packed = w.packed[0].as<u8>() + row0 * (u64)b->stride[0];
  u32 *tok_bucket = w.tok_bucket.as<u32>() + (row0 - tok_row0), *tok_pos = w.tok_pos.as<u32>() + (row0 - tok_row0);
  if (c->walk == SCALCE_WALK_ANCHOR) {
    AnchorArgs g;
    anchor_args(c, b, packed, n, g);
    g.tok_bucket = tok_bucket; g.tok_pos = tok_pos;
    if (cands) {
      g.ntie = ntie; g.tie_read = w.tie_read.as<u32>(); g.tie_off = w.tie_off.as<u32>(); g.bucket_level = c->d_bucket_level.as<u32>();
      g.cand_bucket = w.cand_bucket.as<u32>(); g.cand_pos = w.cand_pos.as<u32>(); g.tie_ncand = w.tie_ncand.as<u32>();
      LAUNCH(tokenize_anchor_k<true>, cdiv(ntie, 256), 256, 0, s, g);
    } else {
      LAUNCH(tokenize_anchor_k<false>, cdiv(n, 256), 256, 0, s, g);
    }
  } else if (cands) {
    TieArgs a;
    a.next = c->d_next.as<uint4>(); a.outinfo = c->d_outinfo.as<u32>(); a.packed = packed; a.L = b->L[0]; a.stride = b->stride[0];
    a.ntie = ntie; a.tie_read = w.tie_read.as<u32>(); a.tie_off = w.tie_off.as<u32>(); a.bucket_level = c->d_bucket_level.as<u32>();
    a.tok_bucket = tok_bucket; a.cand_bucket = w.cand_bucket.as<u32>(); a.cand_pos = w.cand_pos.as<u32>();
    a.tie_ncand = w.tie_ncand.as<u32>();
    a.kmer = c->d_kmer.as<u32>(); a.id8_first = c->id8_first;
    if (t7) LAUNCH(tie_candidates_pipe_k<true>, cdiv(ntie, TOKP_THREADS), TOKP_THREADS, 0, s, a);
    else LAUNCH(tie_candidates_pipe_k<false>, cdiv(ntie, TOKP_THREADS), TOKP_THREADS, 0, s, a);
  } else {
    TokArgs a;
    a.next = c->d_next.as<uint4>(); a.outinfo = c->d_outinfo.as<u32>(); a.packed = packed; a.nrec = n; a.L = b->L[0]; a.stride = b->stride[0];
    a.root_bucket = (u32)c->A.n_buckets; a.tok_bucket = tok_bucket; a.tok_pos = tok_pos;
    a.kmer = c->d_kmer.as<u32>(); a.id8_first = c->id8_first;
    if (t7) LAUNCH(tokenize_kmer_pipe_k<true>, cdiv(n, TOKP_THREADS), TOKP_THREADS, 0, s, a);
    else LAUNCH(tokenize_kmer_pipe_k<false>, cdiv(n, TOKP_THREADS), TOKP_THREADS, 0, s, a);
  }
}

// ---- stage 2: tokenize ------------------------------------------------------------------------------
extern "C" int scalce_batch_tokenize_begin(scalce_batch *b, void *stream) {
  if (!b || !b->ingested[0]) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_TOKENIZE, s);
  // the rows not tokenized yet, [tok_base, N): the piece just appended, or everything when the caller deferred it
  b->tok_base = b->tok_done;
  b->tok_n = b->N - b->tok_done;
  const u64 N = b->tok_n;
  b->jacobi_iters = 0;
  b->tie_fallback = false;
  for (u32 &v : b->tie_plan) v = 0;
  b->sweep_no = 0;
  b->tok_open = true;
  const u32 nb1 = (u32)c->A.n_buckets + 1;  // buckets incl. root
  ENSURE(b, w.tok_bucket, sizeof(u32) * (N + 1));
  ENSURE(b, w.tok_pos, sizeof(u32) * (N + 1));
  ENSURE(b, w.tie_index, sizeof(u32) * (N + 1));
  ENSURE(b, w.ev_off, sizeof(u32) * (N + 1));
  ENSURE(b, w.counts, sizeof(u64) * (nb1 + 1));
  if (!b->counts_total.p) {
    ENSURE(b, b->counts_total, sizeof(u64) * (nb1 + 1));
    ENSURE(b, w.prior_buf, sizeof(u64) * (nb1 + 1));
  }
  if (b->tok_base == 0) HIP_TRY(c, hipMemsetAsync(b->counts_total.p, 0, sizeof(u64) * (nb1 + 1), s));
  ENSURE(b, w.seg, 3 * sizeof(u32) * (nb1 + 2));  // segment starts over all events, over the tie events, fixed reads per bucket
  ENSURE(b, w.Gseg, sizeof(u32) * (nb1 + 2));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(2 * N + 1024) + 1024));
  u32 *ws32 = w.scan_ws.as<u32>();
  ENSURE(b, w.dirty, 2 * sizeof(u32) * (size_t)(nb1 + 64) + sizeof(u64) * (nb1 + 8));
  if (!N) {
    HIP_TRY(c, hipMemsetAsync(w.counts.p, 0, sizeof(u64) * (nb1 + 1), s));
    b->ntie = b->nev = 0;
    return SCALCE_OK;
  }
  // pass A: every read (unless scalce_batch_chunk_plan / scalce_batch_rewindow have walked exactly these rows already: sharded runs)
  if (!(b->tok_base == 0 && b->walk_rows == N && w.walk_owner == b)) launch_walk(b, WALK_FIRST, b->tok_base, N, b->tok_base, s);
  b->walk_rows = 0;  // (the scans below rewrite tok_pos)
  w.walk_owner = nullptr;
  // tie reads: compact, then size the candidate lists by their hit counts
  ENSURE(b, w.tie_read, sizeof(u32) * (N + 1));
  exclusive_scan<u32>(TieFlag{w.tok_pos.as<u32>()}, N,
                      TieCompact{w.tok_pos.as<u32>(), w.tie_index.as<u32>(), w.tie_read.as<u32>()}, ws32, &b->d_scr->ntie, s);
  u32 ntie = 0;
  { int rc = read_u32(b, &b->d_scr->ntie, &ntie, 1, s); if (rc) return rc; }
  // a malformed record (compress.cpp:628-634 exits there) ends the run here, before later stages size anything from its row
  { int rc = check_device_error(b, s); if (rc) { b->tok_open = false; return rc; } }
  b->ntie = ntie;
  ENSURE(b, w.tie_off, sizeof(u32) * (ntie + 2));
  ENSURE(b, w.tie_ncand, sizeof(u32) * (ntie + 2));
  ENSURE(b, w.choice, sizeof(u32) * (ntie + 2));
  u32 ncap = 0;
  if (ntie) {
    exclusive_scan<u32>(TieHits{w.tok_pos.as<u32>(), w.tie_read.as<u32>()}, ntie, StoreTo<u32>{w.tie_off.as<u32>()}, ws32,
                        &b->d_scr->ncand, s);
    int rc = read_u32(b, &b->d_scr->ncand, &ncap, 1, s);
    if (rc) return rc;
  }
  b->ncand_cap = ncap;
  ENSURE(b, w.cand_bucket, sizeof(u32) * (ncap + 2));
  ENSURE(b, w.cand_pos, sizeof(u32) * (ncap + 2));
  ENSURE(b, w.cand_place, sizeof(u32) * (ncap + 2));
  if (ntie) {
    launch_walk(b, WALK_CANDIDATES, b->tok_base, N, b->tok_base, s);
    HIP_TRY(c, hipMemsetAsync(w.choice.p, 0, sizeof(u32) * ntie, s));
  }
  // events in read order, stable-sorted by bucket
  exclusive_scan<u32>(EvCount{w.tok_pos.as<u32>(), w.tie_index.as<u32>(), w.tie_ncand.as<u32>()}, N,
                      StoreTo<u32>{w.ev_off.as<u32>()}, ws32, &b->d_scr->nev, s);
  u32 nev = 0;
  { int rc = read_u32(b, &b->d_scr->nev, &nev, 1, s); if (rc) return rc; }
  b->nev = nev;
  ENSURE(b, w.ev_sorted, sizeof(u32) * (nev + 2));
  ENSURE(b, w.ev_tmp, sizeof(u32) * (nev + 2));
  ENSURE(b, w.ev_place, sizeof(u32) * (nev + 2));
  ENSURE(b, w.chosen, nev + 64);
  ENSURE(b, w.G, sizeof(u32) * (nev + 2));
  ENSURE(b, w.hist, sizeof(u32) * radix_hist_elems(nev > N ? nev : N));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(radix_hist_elems(nev > N ? nev : N)) + scan_ws_elems(nev) + 1024));
  ws32 = w.scan_ws.as<u32>();
  {
    EventArgs a;
    a.nrec = N; a.tok_bucket = w.tok_bucket.as<u32>(); a.tok_pos = w.tok_pos.as<u32>(); a.tie_index = w.tie_index.as<u32>();
    a.tie_off = w.tie_off.as<u32>(); a.tie_ncand = w.tie_ncand.as<u32>(); a.cand_bucket = w.cand_bucket.as<u32>();
    a.ev_off = w.ev_off.as<u32>();
    // the events are sorted by bucket as (key, event) pairs, like the order stage's records (sequential passes; the
    // index-only passes gathered the bucket through the index, and so did the two kernels behind them)
    ENSURE(b, w.key_a, sizeof(u64) * ((size_t)nev + 2));   // (the order stage's 64-bit keys live in the same buffers)
    ENSURE(b, w.key_b, sizeof(u64) * ((size_t)nev + 2));
    a.ev_key = w.key_a.as<u32>();
    LAUNCH(events_fill_k, cdiv(N, 256), 256, 0, s, a);
  }
  int bits = 1;
  while ((1u << bits) < nb1 && bits < 31) bits++;
  const u32 *src = nullptr;  // identity
  u32 *dst = w.ev_sorted.as<u32>(), *alt = w.ev_tmp.as<u32>();
  u32 *ka = w.key_a.as<u32>(), *kb = w.key_b.as<u32>();   // 32-bit keys: bucket << 2 | flags (a third fewer bytes per pass than 64-bit ones)
  for (int sh = 2; sh < 2 + bits; sh += 8) {  // bits 0, 1 (initial flag, tie bit) ride along
    radix_pass_kv(ka, src, kb, dst, nev, (u32)sh, w.hist.as<u32>(), ws32, s);
    src = dst;
    u32 *t = dst; dst = alt; alt = t;
    u32 *tk = ka; ka = kb; kb = tk;
  }
  const u32 *sorted = src;
  // compact view of the tie-candidate events (see events_place_keys_k): what the sweeps work on
  u32 *cidx = dst;  // the ping-pong buffer the sort no longer needs
  exclusive_scan<u32>(TieBitOfKey{ka}, nev, StoreTo<u32>{cidx}, ws32, &b->d_scr->ntev, s);
  u32 ntev = 0;
  { int rc = read_u32(b, &b->d_scr->ntev, &ntev, 1, s); if (rc) return rc; }
  b->ntev = ntev;
  ENSURE(b, w.cand_fixed, sizeof(u32) * (ncap + 2));
  u32 *seg_all = w.seg.as<u32>(), *seg_t = seg_all + (nb1 + 2), *fixed_total = seg_t + (nb1 + 2);
  LAUNCH(events_place_keys_k, cdiv(nev, 256), 256, 0, s, nev, sorted, ka, cidx, w.ev_place.as<u32>(), w.chosen.as<u8>());
  LAUNCH(events_segments_keys_k, cdiv((u64)nev + 1, 256), 256, 0, s, nev, ka, nb1, seg_all);
  LAUNCH(events_compact_segments_k, cdiv(nb1 + 1, 256), 256, 0, s, nb1, seg_all, cidx, nev, ntev, seg_t, fixed_total);
  if (ntie)
    LAUNCH(tie_place_k, cdiv(ntie, 256), 256, 0, s, ntie, w.tie_read.as<u32>(), w.tie_off.as<u32>(), w.tie_ncand.as<u32>(),
           w.ev_off.as<u32>(), w.ev_place.as<u32>(), cidx, w.cand_bucket.as<u32>(), seg_all, seg_t, w.cand_place.as<u32>(),
           w.cand_fixed.as<u32>());
  // first prefix sums (per bucket) and counts; the tie-break follows (scalce_batch_tokenize_settle)
  b->dirty_cur = 0;
  HIP_TRY(c, hipMemsetAsync(w.dirty.p, 0, sizeof(u32) * nb1, s));  // first sweep: every bucket moved "before read 0"
  HIP_TRY(c, hipMemsetAsync(w.dirty.as<u32>() + 2 * (size_t)(nb1 + 64), 0, sizeof(u64) * nb1, s));  // prior seen so far
  if ((u64)ntev < 64ull * nb1)  // fewer than 64 candidate events per bucket on average: a thread per bucket
    LAUNCH(seg_rescan_many_k, cdiv(nb1, 256), 256, 0, s, nb1, seg_t, w.dirty.as<u32>(), w.chosen.as<u8>(), w.G.as<u32>(), fixed_total, w.counts.as<u64>());
  else
    LAUNCH(seg_rescan_k, nb1, 256, 0, s, nb1, seg_t, w.dirty.as<u32>(), w.chosen.as<u8>(), w.G.as<u32>(), fixed_total, w.counts.as<u64>());
  return SCALCE_OK;
}

// The counts a tie-break of rows [tok_base, N) starts from: the caller's cross-shard prior (or none) plus the reads of this
// batch's earlier pieces (bin_size is cumulative, reads.cpp:246).
static const uint64_t *fold_prior(scalce_batch *b, const uint64_t *d_prior, hipStream_t s) {
  if (!b->tok_base) return d_prior;
  scalce_workspace &w = *b->ws;
  if (!d_prior) return b->counts_total.as<uint64_t>();
  const u32 nb1 = (u32)b->ctx->A.n_buckets + 1;
  LAUNCH(add_counts_k, cdiv(nb1, 256), 256, 0, s, nb1, reinterpret_cast<const u64 *>(d_prior), b->counts_total.as<u64>(), w.prior_buf.as<u64>());
  return w.prior_buf.as<uint64_t>();
}

// The global sweeps (SCALCE_TIE_WINDOW=0; the windows of tokenize_windows are the default).  One Jacobi sweep, enqueued
// only: decisions of the tie reads against the current counts, then new prefix sums and per-bucket counts for the buckets
// whose flags moved (seg_rescan_k looks at the dirty marks itself: nothing moved, nothing to do).  flag[0] becomes 1 if any
// decision of this shard moved.  scalce_batch_tokenize_settle sends several out against the same prior counts with ONE
// look at their flags.
static int tokenize_sweep_enqueue(scalce_batch *b, const uint64_t *d_prior, u32 *flag, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  const u32 nb1 = (u32)c->A.n_buckets + 1, ntie = b->ntie;
  d_prior = fold_prior(b, d_prior, s);
  u32 *d0 = w.dirty.as<u32>(), *d1 = d0 + nb1 + 64;
  u32 *dirty_in = b->dirty_cur ? d1 : d0, *dirty_out = b->dirty_cur ? d0 : d1;
  u64 *prior_seen = reinterpret_cast<u64 *>(d0 + 2 * (size_t)(nb1 + 64));
  if (d_prior) LAUNCH(prior_dirty_k, cdiv(nb1, 256), 256, 0, s, nb1, reinterpret_cast<const u64 *>(d_prior), prior_seen, dirty_in);
  HIP_TRY(c, hipMemsetAsync(flag, 0, sizeof(u32), s));
  u32 *G = w.G.as<u32>();
  JacobiArgs a;
  a.ntie = ntie; a.tie_read = w.tie_read.as<u32>(); a.tie_off = w.tie_off.as<u32>(); a.tie_ncand = w.tie_ncand.as<u32>();
  a.cand_bucket = w.cand_bucket.as<u32>(); a.cand_place = w.cand_place.as<u32>(); a.G = G; a.fixed_before = w.cand_fixed.as<u32>();
  a.prior = reinterpret_cast<const u64 *>(d_prior); a.choice = w.choice.as<u32>(); a.chosen = w.chosen.as<u8>();
  a.changed = flag;
  a.dirty_in = dirty_in; a.dirty_out = dirty_out;
  {
    a.coarse = b->sweep_no < 8u ? 1u : 0u;
    b->sweep_no++;
  }
  HIP_TRY(c, hipMemsetAsync(dirty_out, 0xFF, sizeof(u32) * nb1, s));
  LAUNCH(jacobi_k, cdiv(ntie, 256), 256, 0, s, a);
  b->dirty_cur ^= 1;
  LAUNCH(seg_rescan_k, nb1, 256, 0, s, nb1, w.seg.as<u32>() + (nb1 + 2), dirty_out, w.chosen.as<u8>(), G, w.seg.as<u32>() + 2 * (nb1 + 2),
         w.counts.as<u64>());
  return SCALCE_OK;
}

// sweeps allowed before the tie-break gives up sweeping: in all (global sweeps), or per window
static u32 tie_max_sweeps() {
  const char *e = getenv("SCALCE_TIE_MAX_SWEEPS");  // (tests lower it to drive the fallback on ordinary input)
  const int v = e ? atoi(e) : 256;
  return (u32)(v < 1 ? 1 : v);
}
// The tie reads decided in input order by one wavefront (tie_sequential_k): what scalce_batch_tokenize_settle falls back to
// when the sweeps -- of the windows or the global ones -- have not reached their fixed point after tie_max_sweeps() of
// them.  Leaves choice / chosen / G / counts as the converged global sweeps would.
static int tokenize_sequential(scalce_batch *b, const uint64_t *d_prior, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  const u32 nb1 = (u32)c->A.n_buckets + 1, ntie = b->ntie;
  d_prior = fold_prior(b, d_prior, s);
  ENSURE(b, w.Gseg, sizeof(u32) * (nb1 + 2));
  TieSeqArgs a;
  a.ntie = ntie; a.nb1 = nb1; a.tie_off = w.tie_off.as<u32>(); a.tie_ncand = w.tie_ncand.as<u32>(); a.cand_bucket = w.cand_bucket.as<u32>();
  a.fixed_before = w.cand_fixed.as<u32>(); a.prior = reinterpret_cast<const u64 *>(d_prior); a.choice = w.choice.as<u32>();
  a.tiecount = w.Gseg.as<u32>();
  const size_t lds = (size_t)nb1 * 4;
  a.lds_counters = lds <= 100 * 1024 ? 1u : 0u;
  if (!a.lds_counters) HIP_TRY(c, hipMemsetAsync(a.tiecount, 0, sizeof(u32) * nb1, s));
  b->tie_plan[3] = !a.lds_counters ? 3u : lds > 48 * 1024 ? 2u : 1u;
  if (a.lds_counters && lds > 48 * 1024)
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(tie_sequential_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  LAUNCH(tie_sequential_k, 1, 64, a.lds_counters ? lds : 0, s, a);
  HIP_TRY(c, hipMemsetAsync(w.chosen.p, 0, b->nev + 64, s));
  LAUNCH(chosen_from_choice_k, cdiv(ntie, 256), 256, 0, s, ntie, w.tie_off.as<u32>(), w.choice.as<u32>(), w.cand_place.as<u32>(), w.chosen.as<u8>());
  u32 *d0 = w.dirty.as<u32>();
  HIP_TRY(c, hipMemsetAsync(d0, 0, sizeof(u32) * nb1, s));  // every bucket: new prefix sums and counts
  LAUNCH(seg_rescan_k, nb1, 256, 0, s, nb1, w.seg.as<u32>() + (nb1 + 2), d0, w.chosen.as<u8>(), w.G.as<u32>(), w.seg.as<u32>() + 2 * (nb1 + 2),
         w.counts.as<u64>());
  b->tie_fallback = true;
  return SCALCE_OK;
}

// Behind the tie-break: the batch's counts join the run's, and every row gets its bucket, end and tokens (finalize_k).
extern "C" int scalce_batch_tokenize_end(scalce_batch *b, void *stream) {
  if (!b || !b->tok_open) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_TOKENIZE, s);
  b->tok_open = false;
  const u64 N = b->tok_n;
  b->tok_done = b->tok_base + b->tok_n;
  const u32 nb1 = (u32)c->A.n_buckets + 1;
  // reads per bucket over all pieces so far: what the next piece's tie-break starts from, and what the emit stage lays out
  LAUNCH(add_counts_k, cdiv(nb1, 256), 256, 0, s, nb1, w.counts.as<u64>(), b->counts_total.as<u64>(), b->counts_total.as<u64>());
  if (!N) return SCALCE_OK;
  FinalizeArgs a;
  a.nrec = N; a.tok_bucket = w.tok_bucket.as<u32>(); a.tok_pos = w.tok_pos.as<u32>(); a.tie_index = w.tie_index.as<u32>();
  a.tie_off = w.tie_off.as<u32>(); a.choice = w.choice.as<u32>(); a.cand_bucket = w.cand_bucket.as<u32>();
  a.cand_pos = w.cand_pos.as<u32>(); a.bucket_pattern = c->d_bucket_pattern.as<int32_t>(); a.root_bucket = (u32)c->A.n_buckets;
  a.bucket = w.bucket.as<u32>() + b->tok_base; a.end = w.endv.as<u16>() + b->tok_base; a.tokens = w.tokens.as<int32_t>() + 2 * b->tok_base;
  LAUNCH(finalize_k, cdiv(N, 256), 256, 0, s, a);
  return SCALCE_OK;
}

// The tie-break of a batch on its own (fixed prior counts), window by window: see tie_window_sweep_k.  *settled = false
// when the sweeps allowed (tie_max_sweeps() per window) did not get through: the caller decides in input order instead.
static u32 tie_window_reads() {
  const char *e = getenv("SCALCE_TIE_WINDOW");  // tie reads per window; 0 = the global sweeps (jacobi_k)
  const long v = e ? atol(e) : 196608;
  return (u32)(v < 0 ? 0 : v > (1l << 30) ? (1l << 30) : v);
}
// The quality statistics of the shard beside the sweeps (scalce_batch_front asks for it): a few hundred launches of ~13 us on
// at most 192 CUs with nothing between them but their own latency -- 4 ms in which a quarter of the chip counts trigrams on a
// stream of its own (64 workgroups: the sweeps' workgroups and a statistics workgroup do not fit one CU's LDS together, so
// the statistics must leave them their 192 CUs).  The caller's stream joins at the end of the front stages.
extern "C" int scalce_batch_quality(scalce_batch *b, void *stream);
static int quality_beside(scalce_batch *b, hipStream_t s) {
  if (!b->quality_deferred) return SCALCE_OK;
  b->quality_deferred = false;
  scalce_ctx *c = b->ctx;
  if (!b->ws->side) HIP_TRY(c, hipStreamCreateWithFlags(&b->ws->side, hipStreamNonBlocking));
  if (!b->ev_fork) {
    HIP_TRY(c, hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&b->ev_side, hipEventDisableTiming));
  }
  hipStream_t side = b->ws->side;
  HIP_TRY(c, hipEventRecord(b->ev_fork, s));
  HIP_TRY(c, hipStreamWaitEvent(side, b->ev_fork, 0));
  const u32 g = b->tri_grid;
  b->tri_grid = 64;  // (32 / 48 / 64 / 96 / 128 / 256 workgroups: 74.9 / 68.9 / 67.0 / 68.2 / 67.8 / 68.5 ms per shard)
  const int rc = scalce_batch_quality(b, side);
  b->tri_grid = g;
  HIP_TRY(c, hipEventRecord(b->ev_side, side));
  b->side_busy = true;
  return rc;
}
static int tokenize_windows(scalce_batch *b, const uint64_t *d_prior, bool *settled, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  const u32 nb1 = (u32)c->A.n_buckets + 1, ntie = b->ntie, ncap = b->ncand_cap, ntev = b->ntev;
  *settled = false;
  d_prior = fold_prior(b, d_prior, s);
  u32 W = tie_window_reads();
  const u64 max_cells = 64ull << 20;  // (a million-core table: fewer, larger windows)
  if ((u64)cdiv(ntie, W) * nb1 > max_cells) W = (u32)cdiv(ntie, max_cells / nb1 ? max_cells / nb1 : 1);
  const u32 nwin = cdiv(ntie, W);
  b->tie_plan[0] = 2; b->tie_plan[1] = W; b->tie_plan[2] = nwin;  // (two launches per sweep unless the fused kernel takes it below)
  const u64 ncells = (u64)nwin * nb1;
  const u64 nwords = ((u64)ntev >> 6) + 4;
  ENSURE(b, w.tw_cells, sizeof(u32) * (3 * ncells + 8));
  ENSURE(b, w.tw_cand, sizeof(u32) * (2 * (u64)ncap + 8));
  ENSURE(b, w.tw_bits, (sizeof(u64) + sizeof(u32)) * nwords);
  ENSURE(b, w.tw_base, sizeof(u32) * (2 * (u64)nb1 + 64));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(ncells) + 1024));
  u32 *first_delta = w.tw_cells.as<u32>(), *cell_end = first_delta + ncells, *cellstart = cell_end + ncells + 2;  // cellstart[ncells] = all candidates
  u32 *wpos = w.tw_cand.as<u32>(), *rs = wpos + ncap + 2;
  u64 *bits = w.tw_bits.as<u64>();
  u32 *P64 = reinterpret_cast<u32 *>(bits + nwords);
  u32 *base = w.tw_base.as<u32>();
  TieWinState *st = reinterpret_cast<TieWinState *>(base + nb1 + 4);
  const u32 *fixed_total = w.seg.as<u32>() + 2 * (nb1 + 2);
  u32 *key_c = w.G.as<u32>();  // (the global sweeps' prefix sums: not in use here)
  HIP_TRY(c, hipMemsetAsync(first_delta, 0, sizeof(u32) * 2 * ncells, s));  // empty cells: first = end = 0
  HIP_TRY(c, hipMemsetAsync(bits, 0, (sizeof(u64) + sizeof(u32)) * nwords, s));
  HIP_TRY(c, hipMemsetAsync(base, 0, sizeof(u32) * (2 * (u64)nb1 + 64), s));  // (and the state behind it)
  HIP_TRY(c, hipMemsetAsync(w.choice.p, 0xFF, sizeof(u32) * ntie, s));   // nobody has chosen yet
  LAUNCH(tw_key_k, cdiv(ntie, 256), 256, 0, s, ntie, W, nb1, w.tie_off.as<u32>(), w.tie_ncand.as<u32>(), w.cand_bucket.as<u32>(),
         w.cand_place.as<u32>(), key_c);
  if (ntev) LAUNCH(tw_heads_k, cdiv(ntev, 256), 256, 0, s, ntev, key_c, first_delta, cell_end);
  exclusive_scan<u32>(CellCount{first_delta, cell_end}, ncells, StoreTo<u32>{cellstart}, w.scan_ws.as<u32>(), cellstart + ncells, s);
  LAUNCH(tw_delta_k, cdiv(ncells, 256), 256, 0, s, ncells, cellstart, first_delta);
  LAUNCH(tw_cand_k, cdiv(ntie, 256), 256, 0, s, ntie, W, nb1, w.tie_off.as<u32>(), w.tie_ncand.as<u32>(), w.cand_bucket.as<u32>(),
         w.cand_place.as<u32>(), cellstart, first_delta, wpos, rs);
  TieWinArgs a;
  a.ntie = ntie; a.W = W; a.tie_off = w.tie_off.as<u32>(); a.tie_ncand = w.tie_ncand.as<u32>(); a.cand_bucket = w.cand_bucket.as<u32>();
  a.fixed_before = w.cand_fixed.as<u32>(); a.wpos = wpos; a.rs = rs; a.prior = reinterpret_cast<const u64 *>(d_prior); a.base = base;
  a.P64 = P64; a.bits = bits; a.bits32 = reinterpret_cast<u32 *>(bits); a.choice = w.choice.as<u32>(); a.st = st;
  // A window settles in a handful of sweeps when sweeping works at all (the last one moves nothing), so the sweeps go out in
  // batches sized for the windows still open, and the host looks at the device's state once per batch.
  const u64 budget = (u64)tie_max_sweeps() * nwin;
  // one launch per sweep (tie_window_fused_k) when a window's words and their ranks fit a workgroup's LDS
  // (SCALCE_TIE_WINDOW=<reads>:two_launches: test hook -- the path of windows that do not fit)
  const char *tw_env = getenv("SCALCE_TIE_WINDOW");
  if (!(tw_env && strstr(tw_env, ":two_launches"))) {
    TieFusedState *fs = reinterpret_cast<TieFusedState *>(base + 2 * (u64)nb1 + 16);
    u32 *maxw_d = base + 2 * (u64)nb1 + 32;
    LAUNCH(tw_maxwin_k, cdiv(nwin, 256), 256, 0, s, nwin, nb1, cellstart, maxw_d);
    u32 maxw = 0;
    { int rc = read_u32(b, maxw_d, &maxw, 1, s); if (rc) return rc; }
    const size_t lds = (size_t)(maxw + 2) * 12;
    if (lds <= 140 * 1024) {
      b->tie_plan[0] = 1;
      if (lds > 48 * 1024)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(tie_window_fused_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      static const u32 one = 1;
      HIP_TRY(c, hipMemcpyAsync(&fs->changed[2], &one, sizeof(u32), hipMemcpyHostToDevice, s));  // launch 0: "something moved": sweep window 0
      TieFusedArgs g;
      g.a = a; g.nwin = nwin; g.nb1 = nb1; g.lds_words = maxw + 2; g.cellstart = cellstart; g.base2 = base; g.fs = fs;
      const u32 fgrid = cdiv(W < ntie ? W : ntie, TWF_THREADS);
      u32 n = 0;
      TieFusedState h;
      memset(&h, 0, sizeof h);
      { int rc = quality_beside(b, s); if (rc) return rc; }
      for (;;) {
        if (h.sweeps >= budget) { b->jacobi_iters = h.sweeps; return SCALCE_OK; }  // not settled
        const u32 win_now = n ? h.window[(n - 1) & 1] : 0u;
        u64 batch = 4ull * (nwin - win_now) + 4;
        if (batch > 256) batch = 256;
        if (batch > budget - h.sweeps) batch = budget - h.sweeps;
        for (u64 i = 0; i < batch; i++) {
          g.n = n++;
          LAUNCH(tie_window_fused_k, fgrid, TWF_THREADS, lds, s, g);
        }
        int rc = read_u32(b, reinterpret_cast<const u32 *>(fs), reinterpret_cast<u32 *>(&h), 8, s);
        if (rc) return rc;
        if (h.window[(n - 1) & 1] >= nwin) break;
      }
      b->jacobi_iters = h.sweeps;
      LAUNCH(twf_counts_k, cdiv(nb1, 256), 256, 0, s, nb1, fixed_total, base, fs, n - 1, w.counts.as<u64>());
      *settled = true;
      return SCALCE_OK;
    }
  }
  const u32 grid = cdiv(W < ntie ? W : ntie, 256);
  TieWinState h{0, 0, 0, 0};
  while (!h.finished) {
    if (h.sweeps >= budget) { b->jacobi_iters = h.sweeps; return SCALCE_OK; }  // not settled
    u64 batch = 4ull * (nwin - h.window) + 4;
    if (batch > 256) batch = 256;
    if (batch > budget - h.sweeps) batch = budget - h.sweeps;
    for (u64 i = 0; i < batch; i++) {
      LAUNCH(tie_window_sweep_k, grid, 256, 0, s, a);
      LAUNCH(tie_window_tail_k, 1, 1024, 0, s, st, nwin, nb1, cellstart, bits, P64, base);
    }
    int rc = read_u32(b, reinterpret_cast<const u32 *>(st), reinterpret_cast<u32 *>(&h), 4, s);
    if (rc) return rc;
  }
  b->jacobi_iters = h.sweeps;
  LAUNCH(tw_counts_k, cdiv(nb1, 256), 256, 0, s, nb1, fixed_total, base, w.counts.as<u64>());
  *settled = true;
  return SCALCE_OK;
}

extern "C" int scalce_batch_tokenize(scalce_batch *b, const uint64_t *d_prior, void *stream) {
  int rc = scalce_batch_tokenize_begin(b, stream);
  if (rc) return rc;
  return scalce_batch_tokenize_settle(b, d_prior, stream);
}

// The rest of scalce_batch_tokenize behind _begin: the tie-break of this batch on its own (fixed prior counts), then _end.
// (A caller may put other work of the shard beside it; the quality statistics on a second stream were tried twice: no gain.)
extern "C" int scalce_batch_tokenize_settle(scalce_batch *b, const uint64_t *d_prior, void *stream) {
  if (!b || !b->tok_open) return SCALCE_ERR_ARG;
  HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
  int rc;
  if (b->tok_n && b->ntie && tie_window_reads()) {
    hipStream_t ws = (hipStream_t)stream;
    {
      StageTimer tm(b, ST_TOKENIZE, ws);
      bool settled = false;
      if ((rc = tokenize_windows(b, d_prior, &settled, ws))) return rc;
      if (!settled && (rc = tokenize_sequential(b, d_prior, ws))) return rc;
    }
    return scalce_batch_tokenize_end(b, stream);
  }
  // Sweeps go out four at a time and the host looks at their flags once per batch: a sweep after the fixed point changes
  // nothing (and costs next to nothing), while a round trip per sweep left the stream idle 47 times per shard.
  hipStream_t s = (hipStream_t)stream;
  if (b->tok_n && b->ntie) b->tie_plan[0] = 3;
  for (bool done = !(b->tok_n && b->ntie); !done;) {
    StageTimer tm(b, ST_TOKENIZE, s);
    u32 *flags = b->d_scr->sweep_moved;
    for (int i = 0; i < SWEEPS_PER_LOOK; i++)
      if ((rc = tokenize_sweep_enqueue(b, d_prior, flags + i, s))) return rc;
    u32 ch[SWEEPS_PER_LOOK];
    if ((rc = read_u32(b, flags, ch, SWEEPS_PER_LOOK, s))) return rc;
    for (int i = 0; i < SWEEPS_PER_LOOK && !done; i++) {
      b->jacobi_iters++;  // sweeps up to and including the first one that moved nothing, as one at a time would count
      if (!ch[i]) done = true;
    }
    if (!done && b->jacobi_iters >= tie_max_sweeps()) {  // worst cases are quadratic in sweeps: decide in input order instead
      if ((rc = tokenize_sequential(b, d_prior, s))) return rc;
      done = true;
    }
  }
  return scalce_batch_tokenize_end(b, stream);
}

// Sharded runs: where the -B rule (compress.cpp:702-715) cuts this rank's rows, given the bytes already in the chunk that
// is open when they begin.  Record sizes need every row's core LENGTH only (the candidates of a tie are equally long), so
// this runs before the tie-break: the first scan of the tokenizer over all rows, a prefix sum of the sizes, the cuts.
extern "C" int scalce_batch_chunk_plan(scalce_batch *b, uint64_t carry_in, uint64_t *cuts_host, uint32_t cap, uint32_t *ncuts,
                                       uint64_t *carry_out, void *stream) {
  if (!b || !ncuts || !carry_out || (cap && !cuts_host) || !b->ingested[0]) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_TOKENIZE, s);
  const u64 N = b->N;
  *ncuts = 0;
  *carry_out = carry_in;
  if (!N) return SCALCE_OK;
  ENSURE(b, w.tok_bucket, sizeof(u32) * (N + 1));
  ENSURE(b, w.tok_pos, sizeof(u32) * (N + 1));
  if (b->S_rows != N && !(b->tok_done == 0 && b->walk_rows == N && w.walk_owner == b)) {  // (a second call with another carry_in only redoes the cuts)
    launch_walk(b, WALK_FIRST, 0, N, 0, s);
    b->walk_rows = b->tok_done == 0 ? N : 0;  // (tok_bucket / tok_pos are indexed from the first row not tokenized yet)
    w.walk_owner = b;
  }
  ENSURE(b, w.S, sizeof(u64) * (N + 2));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(N + 1) + 1024));
  ENSURE(b, w.chunk_start, sizeof(u64) * (cap + 8));
  u64 *S = w.S.as<u64>();
  if (b->S_rows != N) {
    RecSize rs{w.tok_bucket.as<u32>(), c->d_bucket_level.as<u32>(), w.namelen.as<u8>(), b->L[0], b->L[1], b->p.paired, b->p.use_names, !b->nq};
    exclusive_scan<u64>(rs, N, StoreTo<u64>{S}, w.scan_ws.as<u64>(), S + N, s);
    b->S_rows = N;
  }
  LAUNCH(chunk_cuts_k, 1, 1, 0, s, S, N, (u64)b->p.bucket_set_size, (u64)carry_in, cap, w.chunk_start.as<u64>(), &b->d_scr->ncuts, &b->d_scr->cut_carry);
  u32 n = 0;
  { int rc = read_u32(b, &b->d_scr->ncuts, &n, 1, s); if (rc) return rc; }
  { u64 co = 0; int rc = read_u64(b, &b->d_scr->cut_carry, &co, 1, s); if (rc) return rc; *carry_out = co; }
  if (n) {  // (on the caller's stream: a blocking copy would go through the null stream, which does not wait for `s`)
    HIP_TRY(c, hipMemcpyAsync(cuts_host, w.chunk_start.p, sizeof(u64) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  *ncuts = n;
  return SCALCE_OK;
}

extern "C" int scalce_batch_text_offset(scalce_batch *b, int mate, uint64_t row, uint64_t *offset, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!b || !offset || mate < 0 || mate >= b->nm || row > b->NP) return SCALCE_ERR_ARG;
  if (b->vl) { set_err(b->ctx, "variable-length runs ingest a padded copy of the piece: its offsets are not the caller's"); return SCALCE_ERR_ARG; }
  if (b->keep_comments) { set_err(b->ctx, "a batch that keeps comments is compressed on one GPU: no caller moves its rows"); return SCALCE_ERR_ARG; }
  if (b->keep_bases) { set_err(b->ctx, "a batch that keeps bases is compressed on one GPU: no caller moves its rows"); return SCALCE_ERR_ARG; }
  if (b->keep_plus) { set_err(b->ctx, "a batch that keeps '+' lines is compressed on one GPU: no caller moves its rows"); return SCALCE_ERR_ARG; }
  *offset = 0;
  const u64 line = b->il ? (u64)b->lpr * (2 * row + (u64)mate) : (u64)b->lpr * row;
  if (!line) return SCALCE_OK;  // (-i: mate 2 of row 0 is the text's second record, not its first byte)
  HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
  // from the per-tile newline counts of the piece (its text must still be where it was): no line index is built for this
  const int tm = b->il ? 0 : mate;  // (-i: one text, mate m of row r is its record 2r + m)
  const u64 nbytes = b->text_bytes[tm];
  const u32 ntiles = cdiv(nbytes, IDX_TILE);
  if (!ntiles || !b->piece_text[tm]) { set_err(b->ctx, "no piece ingested"); return SCALCE_ERR_ARG; }
  // on the caller's stream, behind the ingest that produced the tile counts
  u64 *d_out = &b->d_scr->text_offset;
  LAUNCH(line_offset_k, 1, 64, 0, s, b->piece_text[tm], nbytes, b->ws->tile[tm].as<u64>(), ntiles, line, d_out);
  u64 v = 0;
  { int rc = read_u64(b, d_out, &v, 1, s); if (rc) return rc; }
  *offset = v;
  return SCALCE_OK;
}

extern "C" int scalce_batch_set_chunks(scalce_batch *b, const uint64_t *starts, uint32_t n) {
  if (!b || (n && !starts) || n > 4096) return SCALCE_ERR_ARG;
  b->explicit_chunks.assign(starts, starts + n);
  return SCALCE_OK;
}
