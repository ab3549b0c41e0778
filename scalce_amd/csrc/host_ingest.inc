// host_ingest.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): stage 0 (ingest: one piece, appended pieces, a moved window of rows) and stage 1 (quality statistics)
// ---- stage 0: ingest ------------------------------------------------------------------------------
// newline count of one mate's text; the per-tile bases stay in the workspace's tile[mate] for piece_unpack
static int piece_count(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, hipStream_t s, u64 *nlines, u8 *last) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  if (((uintptr_t)d_text & 15) != 0) { set_err(c, "FASTQ text must be 16-byte aligned"); return SCALCE_ERR_ARG; }
  if (nbytes > b->max_text) b->max_text = nbytes;  // max_text only sizes the first allocations; everything below grows
  b->text_bytes[mate] = nbytes;
  const u32 ntiles = cdiv(nbytes, IDX_TILE);
  ENSURE(b, w.tile[mate], (ntiles + 8) * sizeof(u64));
  ENSURE(b, w.scan_ws, (scan_ws_elems(ntiles) + 64) * sizeof(u64));
  u64 *tile = w.tile[mate].as<u64>();  // [ntiles] counts -> bases
  *nlines = 0;
  *last = '\n';
  if (ntiles) {
    LAUNCH(index_count_k, ntiles, IDX_THREADS, 0, s, d_text, nbytes, tile);
    exclusive_scan<u64>(LoadAs<u64, u64>{tile}, ntiles, StoreTo<u64>{tile}, w.scan_ws.as<u64>(), &b->d_scr->nlines[mate], s);
    HIP_TRY(c, hipMemcpyAsync(nlines, &b->d_scr->nlines[mate], sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost, s));
  }
  return SCALCE_OK;
}

// the line index of the piece (index_write_k), built when something needs it: the indexed unpack kernels, names longer
// than a cell, scalce_batch_text_offset (interleaved: mate 0's, which is both mates')
static int ensure_line_index(scalce_batch *b, int mate, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  if (b->line_index_ok[mate]) return SCALCE_OK;
  const u64 nrec = b->NP, nbytes = b->text_bytes[mate];
  if (nrec > w.piece_rows_cap || !w.line_end[mate].p) {
    if (nrec > w.piece_rows_cap) w.piece_rows_cap = nrec;
    ENSURE(b, w.line_end[mate], sizeof(u64) * b->unit_lines() * (w.piece_rows_cap + 1));
  }
  const u32 ntiles = cdiv(nbytes, IDX_TILE);
  if (ntiles) LAUNCH(index_write_k, ntiles, IDX_THREADS, 0, s, b->piece_text[mate], nbytes, w.tile[mate].as<u64>(), w.line_end[mate].as<u64>(), b->unit_lines() * nrec);
  b->line_index_ok[mate] = true;
  return SCALCE_OK;
}

// --keep-comments: what follows the name on the header lines of the piece's first `nrec` rows goes behind mate m's entries of
// earlier pieces (com_in[m], input order), each entry with its newline; comlen[m] keeps the lengths per row.  Runs behind the
// rows' own ingest (mate 0's lengths come from namelen), from the piece's line index: a plan pass, one exclusive scan, one
// copy pass.  The text is not needed again.  `mate`: the text's; an interleaved text (mate 0's) serves both mates.
static int piece_comments(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  { int rc = ensure_line_index(b, mate, s); if (rc) return rc; }
  ENSURE(b, b->com_piece_off, sizeof(u64) * (nrec + 8));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nrec) + 64));
  for (int m = mate; m < (b->il ? 2 : mate + 1); m++) {
    const u64 rows = std::max<u64>(w.row_cap, b->base + nrec);
    { int rc = ensure_keep(b, b->comlen[m], sizeof(u16) * (rows + 64), sizeof(u16) * b->base, s); if (rc) return rc; }
    if (b->base == 0) HIP_TRY(c, hipMemsetAsync(&b->d_scr->comment_longest[m], 0, sizeof(u32), s));
    CommentArgs a;
    a.text = d_text; a.nbytes = nbytes; a.line_end = w.line_end[mate].as<u64>();
    a.unit_lines = (u32)b->unit_lines(); a.line0 = m == mate ? 0u : (u32)b->lpr;
    a.nrec = nrec; a.row0 = b->base;
    a.namelen = m == 0 ? w.namelen.as<u8>() + b->base : nullptr;
    a.comlen = b->comlen[m].as<u16>() + b->base;
    a.off = b->com_piece_off.as<u64>();
    a.dst = nullptr;
    a.longest = &b->d_scr->comment_longest[m];
    a.err = b->d_err;
    LAUNCH(comment_plan_k, cdiv(nrec, 256), 256, 0, s, a);
    exclusive_scan<u64>(CommentSize{a.comlen}, nrec, StoreTo<u64>{a.off}, w.scan_ws.as<u64>(), a.off + nrec, s);
    { int rc = check_device_error(b, s); if (rc) return rc; }
    u64 total = 0;
    { int rc = read_u64(b, a.off + nrec, &total, 1, s); if (rc) return rc; }
    { int rc = read_u32(b, &b->d_scr->comment_longest[m], &b->com_longest[m], 1, s); if (rc) return rc; }
    { int rc = ensure_keep(b, b->com_in[m], b->com_used[m] + total + 64, b->com_used[m], s); if (rc) return rc; }
    a.dst = b->com_in[m].as<u8>() + b->com_used[m];
    LAUNCH(comment_copy_k, cdiv(total, COM_SPAN), 256, 0, s, a);
    b->com_used[m] += total;
  }
  return SCALCE_OK;
}

// --keep-plus: the third lines of the piece's first `nrec` rows, as entries (kernels_plus.hpp), go behind mate m's entries of
// earlier pieces (plus_in[m], input order); pluslen[m] keeps the stored lengths per row.  The shape of piece_comments: a plan
// pass (class and length; the two errors of the option), one exclusive scan of length + 1, one extract pass.
static int piece_plus(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  { int rc = ensure_line_index(b, mate, s); if (rc) return rc; }
  ENSURE(b, b->com_piece_off, sizeof(u64) * (nrec + 8));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nrec) + 64));
  for (int m = mate; m < (b->il ? 2 : mate + 1); m++) {
    const u64 rows = std::max<u64>(w.row_cap, b->base + nrec);
    { int rc = ensure_keep(b, b->pluslen[m], sizeof(u16) * (rows + 64), sizeof(u16) * b->base, s); if (rc) return rc; }
    if (b->base == 0) HIP_TRY(c, hipMemsetAsync(&b->d_scr->plus_longest[m], 0, sizeof(u32), s));
    CommentArgs a;
    a.text = d_text; a.nbytes = nbytes; a.line_end = w.line_end[mate].as<u64>();
    a.unit_lines = (u32)b->unit_lines(); a.line0 = m == mate ? 0u : (u32)b->lpr;
    a.nrec = nrec; a.row0 = b->base;
    a.namelen = nullptr;
    a.comlen = b->pluslen[m].as<u16>() + b->base;
    a.off = b->com_piece_off.as<u64>();
    a.dst = nullptr;
    a.longest = &b->d_scr->plus_longest[m];
    a.err = b->d_err;
    LAUNCH(plus_plan_k, cdiv(nrec, 256), 256, 0, s, a);
    exclusive_scan<u64>(CommentSize{a.comlen}, nrec, StoreTo<u64>{a.off}, w.scan_ws.as<u64>(), a.off + nrec, s);
    { int rc = check_device_error(b, s); if (rc) return rc; }
    u64 total = 0;
    { int rc = read_u64(b, a.off + nrec, &total, 1, s); if (rc) return rc; }
    { int rc = read_u32(b, &b->d_scr->plus_longest[m], &b->plus_longest[m], 1, s); if (rc) return rc; }
    { int rc = ensure_keep(b, b->plus_in[m], b->plus_used[m] + total + 64, b->plus_used[m], s); if (rc) return rc; }
    a.dst = b->plus_in[m].as<u8>() + b->plus_used[m];
    LAUNCH(plus_copy_k, cdiv(total, COM_SPAN), 256, 0, s, a);
    b->plus_used[m] += total;
  }
  return SCALCE_OK;
}

// --keep-bases: the exceptions of the piece's first `nrec` rows (kernels_exceptions.hpp) go behind mate m's entries of earlier
// pieces (exc_in[m], input order); exc_cnt[m] keeps the count per row.  Runs behind the rows' own ingest, from the piece's line
// index and over the text the ingest read: a count pass, one exclusive scan and, when the piece has any, a write pass.
// `mate`: the text's; an interleaved text (mate 0's) serves both mates.
static int piece_exceptions(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  { int rc = ensure_line_index(b, mate, s); if (rc) return rc; }
  const u32 nblocks = cdiv(nrec, EXC_ROWS);
  ENSURE(b, b->exc_piece_off, sizeof(u64) * (nrec + 8) + sizeof(u32) * ((size_t)nblocks + 8));  // (offsets, total, rows; the workgroups' rows)
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nrec) + 64));
  for (int m = mate; m < (b->il ? 2 : mate + 1); m++) {
    const u64 rows = std::max<u64>(w.row_cap, b->base + nrec);
    { int rc = ensure_keep(b, b->exc_cnt[m], sizeof(u16) * (rows + 64), sizeof(u16) * b->base, s); if (rc) return rc; }
    ExcArgs a;
    a.text = d_text; a.nbytes = nbytes; a.line_end = w.line_end[mate].as<u64>();
    a.lpr = (u32)b->lpr; a.unit_recs = b->il ? 2u : 1u; a.rec0 = m == mate ? 0u : 1u;
    a.L = (u32)b->L[m];
    a.has_q = b->nq ? 0u : 1u;
    a.q_affine = b->nq ? -1 : b->q_affine[m];
    a.qzero[0] = a.qzero[1] = 0;
    a.qzero_end = 0;
    for (int i = 0; i < 128 && !b->nq; i++)
      if (b->p.qmap[m].values[i] == b->p.qmap[m].offset) { a.qzero[i >> 6] |= 1ull << (i & 63); a.qzero_end = (u32)i + 1; }
    a.qlut = b->nq ? nullptr : b->d_qlut[m];
    a.qoffset = b->nq ? 0u : (u32)b->p.qmap[m].offset & 255u;
    a.padlen = b->vl ? w.padlen[m].as<u16>() + b->base : nullptr;
    a.nrec = nrec;
    a.count = b->exc_cnt[m].as<u16>() + b->base;
    a.off = b->exc_piece_off.as<u64>();
    a.dst = nullptr;
    a.rows_with = reinterpret_cast<u32 *>(b->exc_piece_off.as<u64>() + nrec + 8);
    LAUNCH(exc_count_k, nblocks, 256, 0, s, a);
    exclusive_scan<u64>(ExcCount{a.count}, nrec, StoreTo<u64>{b->exc_piece_off.as<u64>()}, w.scan_ws.as<u64>(), b->exc_piece_off.as<u64>() + nrec, s);
    // (the rows that hold one: the sum of the workgroups' counts, into the word behind the total -- read back with it)
    exclusive_scan<u64>(LoadAs<u32, u64>{a.rows_with}, nblocks, ExcNoStore{}, w.scan_ws.as<u64>(), b->exc_piece_off.as<u64>() + nrec + 1, s);
    u64 back[2] = {0, 0};  // the piece's entries, its rows that hold one
    { int rc = read_u64(b, a.off + nrec, back, 2, s); if (rc) return rc; }
    const u64 total = back[0];
    b->exc_rows[m] += back[1];
    if (!total) continue;
    { int rc = ensure_keep(b, b->exc_in[m], sizeof(u64) * (b->exc_used[m] + total + 8), sizeof(u64) * b->exc_used[m], s); if (rc) return rc; }
    a.dst = b->exc_in[m].as<u64>() + b->exc_used[m];
    LAUNCH(exc_write_k, cdiv(nrec, EXC_ROWS), 256, 0, s, a);
    b->exc_used[m] += total;
  }
  return SCALCE_OK;
}

// the first `nrec` records of the text -> rows [base, base + nrec): 2-bit bases, q', names
// (A one-pass variant -- no count pass, the tiles' line bases by decoupled look-back between the workgroups -- was byte-exact
// and slower: 9.2 ms against 1.7 + 6.2 at 50 M x 100 bp, rounds 3-4; removed in round 5.)
// which kernel wrote a mate's rows (scalce_batch_ingest_plan, scalce_hip.h)
enum IngestKernel : u32 { INGK_NONE = 0, INGK_ONE_PASS = 1, INGK_TILED = 2, INGK_DIRECT = 3 };
// LPR = lines per record, QOUT = q' rows written, IL = interleaved pairs: the record variants of the kernels (unpack_record_at).
// IL: called for mate 0 with the one text, which it ingests for both mates -- nrec pairs, one count, one line index.
template <int LPR, bool QOUT, bool IL>
static int piece_unpack_t(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  scalce_workspace &w = *b->ws;
  constexpr auto k_tiles2 = &ingest_tiles2_k<LPR, QOUT, IL>;
  constexpr auto k_unpack_tiled = &unpack_tiled_k<LPR, QOUT, IL>;
  constexpr auto k_unpack = &unpack_k<LPR, QOUT, IL>;
  constexpr auto k_last_end = &last_record_end_k<LPR, IL>;
  constexpr auto k_long_names = &long_names_k<LPR, IL>;
  constexpr int NMATE = IL ? 2 : 1;
  scalce_ctx *c = b->ctx;
  for (int m = mate; m < mate + NMATE; m++) {
    b->piece_text[m] = d_text;
    b->text_bytes[m] = nbytes;
    b->line_index_ok[m] = false;
    b->piece_consumed[m] = 0;
    for (int i = 0; i < 4; i++) b->ingest_plan[m][i] = 0;
  }
  if (!nrec) return SCALCE_OK;
  // the arguments of the launches that write mate m's rows
  auto args_of = [&](int m) {
    UnpackArgs a;
    a.text = d_text; a.nbytes = nbytes; a.line_end = nullptr; a.nrec = nrec;
    a.L = b->L[m]; a.stride = b->stride[m]; a.mate = m; a.use_names = b->p.use_names; a.no_ac = b->p.no_ac;
    a.packed = w.packed[m].as<u8>() + b->base * (u64)b->stride[m];
    a.q = QOUT ? w.q[m].as<u8>() + b->base * (u64)b->qstride[m] : nullptr;
    a.qstride = b->qstride[m];
    a.cellstride = 16;
    a.packed2 = nullptr;
    a.namelen = w.namelen.as<u8>() + b->base;
    a.namecell = (m == 0 && b->p.use_names) ? w.namecell.as<u8>() + 16 * b->base : nullptr;
    a.qlut = b->d_qlut[m]; a.err = b->d_err;
    a.q_affine = b->q_affine[m];
    a.max_namelen = &b->d_scr->ingest.max_namelen;
    return a;
  };
  UnpackArgs a = args_of(mate);
  const bool fused_rows = b->fused && mate == 0;  // (never under IL: fused rows are single-end)
  if (fused_rows) a.packed2 = a.q + b->row_cell_off;  // a copy of the packed words lies behind the row's q'
  BatchScratch::IngestFlags *d_flags = &b->d_scr->ingest;  // mate 0 finds the longest name; every text may turn out slow
  u32 *slow = &d_flags->slow;
  u64 *d_consumed = &b->d_scr->consumed[mate];
  if (mate == 0) HIP_TRY(c, hipMemsetAsync(d_flags, 0, sizeof *d_flags, s));
  else HIP_TRY(c, hipMemsetAsync(slow, 0, sizeof(u32), s));
  // one pass behind the count for the usual read lengths (ingest_tiles2_k); the indexed kernels otherwise, and when a
  // record turns out not to fit the tile overlap
  bool fused = a.L >= 16 && a.L <= 160 && !getenv("SCALCE_INGEST_INDEXED");
  BatchScratch::IngestFlags flags = {0, 0};
  for (int m = mate; m < mate + NMATE; m++) b->mm_valid[m] = false;
  if (IL) fused = fused && b->L[1] >= 16 && b->L[1] <= 160;
  if (fused) {
    const u32 ntiles2 = cdiv(nbytes, ING_TILE);
    // one launch: mate `mate`'s arguments, and under IL mate 2's beside them (the kernel ignores the second set otherwise)
    Ingest2Args ga[2];
    for (int i = 0; i < NMATE; i++) {
      const int m = mate + i;
      IngestArgs ia;
      ia.u = i ? args_of(m) : a;
      ia.tile_base = w.tile[mate].as<u64>();
      ia.consumed = d_consumed;
      ia.slow = slow;
      if (QOUT) ENSURE(b, w.tile_mm[m], sizeof(u16) * ((size_t)ntiles2 + 8));
      Ingest2Args &g = ga[i];
      g.i = ia;
      const u64 S = (u64)ia.u.stride / 4, W = ((u64)ia.u.L + 15) / 16;
      g.magic_s = ((1ull << 32) + S - 1) / S;
      g.magic_w = ((1ull << 32) + W - 1) / W;
      g.step_ks = (u32)(ING_THREADS / S); g.step_rs = (u32)(ING_THREADS % S);
      g.step_kw = (u32)(ING_THREADS / W); g.step_rw = (u32)(ING_THREADS % W);
      g.tile_minmax = QOUT ? w.tile_mm[m].as<u16>() : nullptr;
    }
    if (!IL) ga[1] = ga[0];
    LAUNCH(k_tiles2, ntiles2, ING_THREADS, 0, s, ga[0], ga[1]);
    if (QOUT)
      for (int m = mate; m < mate + NMATE; m++) {
        b->mm_valid[m] = true;
        w.tile_mm_owner[m] = b;
      }
    { int rc = read_words(b, d_flags, &flags, sizeof flags / 4, s); if (rc) return rc; }
    for (int m = mate; m < mate + NMATE; m++) b->ingest_plan[m][0] = INGK_ONE_PASS;
    if (flags.slow) {  // a record longer than the overlap: redo the piece the indexed way
      fused = false;
      for (int m = mate; m < mate + NMATE; m++) { b->mm_valid[m] = false; b->ingest_plan[m][1] = 1; }
    }
  }
  if (!fused) {
    { int rc = ensure_line_index(b, mate, s); if (rc) return rc; }
    a.line_end = w.line_end[mate].as<u64>();
    if (mate == 0) HIP_TRY(c, hipMemsetAsync(&d_flags->max_namelen, 0, sizeof(u32), s));
    u8 *row_q = a.q;
    if (fused_rows) {  // the indexed kernels write rows back to back: into an array of the piece's own, fused behind them
      ENSURE(b, b->fuse_q, (size_t)a.L * nrec + 64);
      a.q = b->fuse_q.as<u8>();
      a.qstride = (u32)a.L;
      a.packed2 = nullptr;
    }
    for (int m = mate; m < mate + NMATE; m++) {  // (IL: mate 2 from the same text and line index)
      UnpackArgs am = a;
      if (m != mate) { am = args_of(m); am.line_end = a.line_end; }
      const bool tiled = (size_t)UNP_RPB * am.L <= (size_t)UNP_Q_CAP;
      b->ingest_plan[m][0] = tiled ? INGK_TILED : INGK_DIRECT;
      if (tiled) LAUNCH(k_unpack_tiled, cdiv(nrec, UNP_RPB), 2 * UNP_RPB, unp_text_cap(am.L) + 32 + (QOUT ? unp_q_cap(am.L) : 0u), s, am);
      else LAUNCH(k_unpack, cdiv(nrec, 256), 256, 0, s, am);
    }
    if (fused_rows)
      LAUNCH(fuse_rows_k, cdiv(nrec, 256), 256, 0, s, nrec, b->fuse_q.as<u8>(), (u32)a.L, (const u8 *)nullptr, a.packed, (u32)a.stride, b->row_pwords,
             row_q, b->qstride[0], b->row_cell_off);
    LAUNCH(k_last_end, 1, 1, 0, s, a.line_end, nrec, d_consumed);
    { int rc = read_u32(b, &d_flags->max_namelen, &flags.max_namelen, 1, s); if (rc) return rc; }
  }
  { u64 v = 0; int rc = read_u64(b, d_consumed, &v, 1, s); if (rc) return rc; b->piece_consumed[mate] = v; }
  if (mate == 0 && b->p.use_names) {
    // names that do not fit their 16-byte cell go to the long-name store (input order): the text is not needed again
    const u32 maxlen = flags.max_namelen;
    if (maxlen > 15) {
      { int rc = ensure_line_index(b, mate, s); if (rc) return rc; }
      if (!w.name_in_off.p) {
        ENSURE(b, w.name_in_off, sizeof(u64) * (w.row_cap + 2));
        HIP_TRY(c, hipMemsetAsync(w.name_in_off.p, 0, sizeof(u64) * (w.row_cap + 2), s));
      }
      ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nrec) + 64));
      u64 *off = w.name_in_off.as<u64>() + b->base;
      exclusive_scan<u64>(LongNameLen{a.namelen}, nrec, StoreTo<u64>{off}, w.scan_ws.as<u64>(), &b->d_scr->long_names_bytes, s);
      u64 total = 0;
      { int rc = read_u64(b, &b->d_scr->long_names_bytes, &total, 1, s); if (rc) return rc; }
      { int rc = ensure_keep(b, w.names_in, b->names_in_used + total + 64, b->names_in_used, s); if (rc) return rc; }
      LAUNCH(k_long_names, cdiv(nrec, 256), 256, 0, s, nrec, d_text, w.line_end[mate].as<u64>(), a.namelen, off, b->names_in_used, w.names_in.as<u8>());
      b->names_in_used += total;
      b->ingest_plan[mate][3] = (u32)total;
    }
  }
  if (b->keep_comments) { int rc = piece_comments(b, mate, d_text, nbytes, nrec, s); if (rc) return rc; }
  if (b->keep_bases) { int rc = piece_exceptions(b, mate, d_text, nbytes, nrec, s); if (rc) return rc; }
  if (b->keep_plus) { int rc = piece_plus(b, mate, d_text, nbytes, nrec, s); if (rc) return rc; }
  b->ingest_plan[mate][2] = b->line_index_ok[mate] ? 1u : 0u;
  if (IL)  // (one text, one line index, mate 1's names: mate 2 reports what mate 1 does, and the kernel that wrote its own rows)
    for (int i = 1; i < 4; i++) b->ingest_plan[mate + 1][i] = b->ingest_plan[mate][i];
  return SCALCE_OK;
}
template <bool IL>
static int piece_unpack_il(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  if (b->lpr == 2) return piece_unpack_t<2, false, IL>(b, mate, d_text, nbytes, nrec, s);  // -f
  if (b->nq) return piece_unpack_t<4, false, IL>(b, mate, d_text, nbytes, nrec, s);        // -Q
  return piece_unpack_t<4, true, IL>(b, mate, d_text, nbytes, nrec, s);
}
// interleaved: both mates' rows from the one text (mate 0's call); nrec counts pairs
static int piece_unpack(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s) {
  return b->il ? piece_unpack_il<true>(b, mate, d_text, nbytes, nrec, s) : piece_unpack_il<false>(b, mate, d_text, nbytes, nrec, s);
}
// Variable-length runs: the first `nrec` records of the caller's piece (piece_count has left its tiles' line bases in tile[mate])
// become the padded text the ingest kernels read -- every read 'N' up to L, every quality line the offset character up to L --
// in the workspace, and L - length goes into the row array padlen[mate] at the piece's rows.  The line index of the piece,
// one plan pass per record (lengths checked: a record beyond L or with lines that differ ends the call with SCALCE_ERR_FORMAT),
// one exclusive scan of the padded sizes, one copy pass; the buffer is sized from the scan's total: a piece of short reads grows.
// *used = bytes of the caller's piece those records take.  The padded text is then counted like any piece (piece_count).
static int pad_piece(scalce_batch *b, int mate, const u8 *d_text, u64 nbytes, u64 nrec, hipStream_t s, const u8 **padded, u64 *padded_bytes,
                     u64 *used) {
  scalce_workspace &w = *b->ws;
  scalce_ctx *c = b->ctx;
  ENSURE(b, w.vl_line_end[mate], sizeof(u64) * (4 * nrec + 8));
  ENSURE(b, w.vl_off[mate], sizeof(u64) * (nrec + 8));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nrec) + 64));
  PadArgs a;
  a.text = d_text; a.nbytes = nbytes; a.nrec = nrec; a.row0 = b->base;
  a.line_end = w.vl_line_end[mate].as<u64>();
  a.L = (u32)b->L[mate];
  a.qpad = (u32)b->p.qmap[mate].offset & 127u;
  a.padlen = w.padlen[mate].as<u16>() + b->base;
  a.dst_off = w.vl_off[mate].as<u64>();
  a.dst = nullptr;
  a.err = b->d_err;
  LAUNCH(index_write_k, cdiv(nbytes, IDX_TILE), IDX_THREADS, 0, s, d_text, nbytes, w.tile[mate].as<u64>(), w.vl_line_end[mate].as<u64>(), 4 * nrec);
  LAUNCH(pad_plan_k, cdiv(nrec, 256), 256, 0, s, a);
  exclusive_scan<u64>(PaddedSize{a.line_end, a.padlen}, nrec, StoreTo<u64>{a.dst_off}, w.scan_ws.as<u64>(), a.dst_off + nrec, s);
  b->vl_mate = mate;
  { int rc = check_device_error(b, s); if (rc) return rc; }
  u64 total = 0, last_end = 0;
  { int rc = read_u64(b, a.dst_off + nrec, &total, 1, s); if (rc) return rc; }
  { int rc = read_u64(b, a.line_end + 4 * nrec - 1, &last_end, 1, s); if (rc) return rc; }
  ENSURE(b, w.vl_text[mate], (size_t)total + 256);
  a.dst = w.vl_text[mate].as<u8>();
  LAUNCH(pad_copy_k, cdiv(total, VL_SPAN), 256, 0, s, a);
  u64 nlines = 0;
  u8 last = 0;
  { int rc = piece_count(b, mate, a.dst, total, s, &nlines, &last); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (nlines != 4 * nrec || last != '\n') { set_err(c, "internal: the padded text of %llu records has %llu lines", (unsigned long long)nrec, (unsigned long long)nlines); return SCALCE_ERR_HIP; }
  *padded = a.dst;
  *padded_bytes = total;
  *used = last_end + 1;
  return SCALCE_OK;
}

// "(ERROR) ..." for a text whose line count does not make whole records (pairs, under -i)
static int text_shape_error(scalce_batch *b, u64 nlines, u8 last) {
  const u64 lpr = (u64)b->lpr;
  if (b->il && nlines % lpr == 0 && last == '\n')
    set_err(b->ctx, "(ERROR) interleaved text holds an odd number of records (%llu): every mate-1 record must be followed by its mate 2",
            (unsigned long long)(nlines / lpr));
  else
    set_err(b->ctx, "(ERROR) %s text has %llu lines (not a multiple of %d) or no trailing newline", b->lpr == 2 ? "FASTA" : "FASTQ",
            (unsigned long long)nlines, b->lpr);
  return SCALCE_ERR_FORMAT;
}

static void batch_restart(scalce_batch *b) {
  b->N = b->base = b->NP = 0;
  b->S_rows = ~0ull;
  b->walk_rows = 0;
  b->tok_done = b->tok_base = b->tok_n = 0;
  b->appending = false;
  b->names_in_used = 0;
  for (int m = 0; m < 2; m++) b->com_used[m] = b->out_comments_bytes[m] = b->com_longest[m] = 0;
  for (int m = 0; m < 2; m++) b->exc_used[m] = b->exc_rows[m] = b->out_exc_entries[m] = 0;
  for (int m = 0; m < 2; m++) { b->plus_used[m] = b->out_plus_bytes[m] = 0; b->plus_longest[m] = b->plus_repeats[m] = b->plus_literals[m] = 0; }
  b->tri_expected[0] = b->tri_expected[1] = 0;
  b->ingested[0] = b->ingested[1] = false;
  for (int m = 0; m < 2; m++)
    for (int i = 0; i < 4; i++) b->ingest_plan[m][i] = 0;
  // (frames laid out but not copied belong to the shard that is being replaced: scalce_batch_qual_window must not serve them)
  for (int m = 0; m < 2; m++) { b->frame_virtual[m] = 0; b->frame_off_host[m].clear(); }
}

extern "C" int scalce_batch_reset(scalce_batch *b) {
  if (!b) return SCALCE_ERR_ARG;
  batch_restart(b);
  return SCALCE_OK;
}

extern "C" int scalce_batch_ingest(scalce_batch *b, int mate, const uint8_t *d_text, uint64_t nbytes, void *stream) {
  if (!b || mate < 0 || mate >= b->nm || !d_text) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  if (mate >= b->ntext) { set_err(c, "interleaved batch: both mates come in one text, ingested as mate 0"); return SCALCE_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_INGEST, s);
  if (mate == 0) batch_restart(b);  // one piece = the whole shard
  u64 nlines = 0;
  u8 last = '\n';
  { int rc = piece_count(b, mate, d_text, nbytes, s, &nlines, &last); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(s));
  if ((nlines % b->unit_lines()) || last != '\n') return text_shape_error(b, nlines, last);
  const u64 nrec = nlines / b->unit_lines();  // (records; pairs under -i)
  if (nrec > b->max_reads) { set_err(c, "%llu records exceed the batch capacity", (unsigned long long)nrec); return SCALCE_ERR_CAPACITY; }
  if (mate == 0) { b->N = b->NP = nrec; }
  else if (nrec != b->N) { set_err(c, "(ERROR) mates have different record counts"); return SCALCE_ERR_FORMAT; }
  u64 used = 0;
  if (b->vl && nrec) {  // (the ingest reads the padded text)
    u64 padded_bytes = 0;
    int rc = pad_piece(b, mate, d_text, nbytes, nrec, s, &d_text, &padded_bytes, &used);
    if (rc) return rc;
    nbytes = padded_bytes;
  }
  { int rc = piece_unpack(b, mate, d_text, nbytes, nrec, s); if (rc) return rc; }
  b->ingested[mate] = true;
  if (b->il) b->ingested[1] = true;
  return SCALCE_OK;
}

// Streaming form of the record reader: the next piece of the read stream goes BEHIND the rows the batch already holds.
// As many complete records as both mates' pieces hold are taken (compress.cpp:614-666 reads the mates in step);
// consumed[m] says how many bytes of each piece that was, the caller hands the rest in again in front of the next
// piece.  Ingest, quality counters and the tie-break of the new rows (against all rows before them) run here; order,
// emit and entropy run once, over everything, when the caller has no more input.
static int entropy_rerun_from_text(scalce_batch *b, hipStream_t s);
enum WalkPass { WALK_FIRST, WALK_CANDIDATES };
static void launch_walk(scalce_batch *b, WalkPass pass, u64 row0, u64 n, u64 tok_row0, hipStream_t s);  // (host_tokenize.inc)
// the ingest half of scalce_batch_append: as many complete records as both mates' pieces hold -> rows [N, N + nrec)
static int ingest_piece(scalce_batch *b, const uint8_t *const text[2], const u64 nbytes[2], bool final_piece, uint64_t consumed[2], hipStream_t s) {
  scalce_ctx *c = b->ctx;
  consumed[0] = consumed[1] = 0;
  u64 nlines[2] = {0, 0}, nrec = ~0ull;
  u8 last[2] = {'\n', '\n'};
  StageTimer tm(b, ST_INGEST, s);
  for (int m = 0; m < b->ntext; m++)
    if (nbytes[m]) { int rc = piece_count(b, m, text[m], nbytes[m], s, &nlines[m], &last[m]); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(s));
  const u64 lpr = b->unit_lines();  // (a pair's lines under -i: pieces end on a pair boundary)
  for (int m = 0; m < b->ntext; m++) nrec = nlines[m] / lpr < nrec ? nlines[m] / lpr : nrec;
  if (final_piece) {
    for (int m = 0; m < b->ntext; m++)
      if ((nlines[m] % lpr) || last[m] != '\n') return text_shape_error(b, lpr * b->N + nlines[m], last[m]);
    if (b->ntext == 2 && nlines[0] != nlines[1]) { set_err(c, "(ERROR) mates have different record counts"); return SCALCE_ERR_FORMAT; }
  }
  b->base = b->N;
  b->NP = nrec;
  if (b->base + nrec >= (1ull << 32) - 64) { set_err(c, "a batch holds fewer than 2^32 reads"); return SCALCE_ERR_CAPACITY; }
  { int rc = reserve_rows(b, b->base + nrec, b->base, s); if (rc) return rc; }
  for (int m = 0; m < b->ntext; m++) {
    const u8 *t = text[m];
    u64 tn = nbytes[m], used = 0;
    if (b->vl && nrec) { int rc = pad_piece(b, m, t, tn, nrec, s, &t, &tn, &used); if (rc) return rc; }  // (consumed stays in the caller's bytes)
    int rc = piece_unpack(b, m, t, tn, nrec, s);
    if (rc) return rc;
    b->ingested[m] = true;
    consumed[m] = nrec ? (b->vl ? used : b->piece_consumed[m]) : 0;  // behind the newline that ends the last record taken
  }
  if (b->il) b->ingested[1] = true;
  HIP_TRY(c, hipStreamSynchronize(s));
  b->N = b->base + nrec;
  return SCALCE_OK;
}

extern "C" int scalce_batch_append(scalce_batch *b, const uint8_t *d_text1, uint64_t n1, const uint8_t *d_text2, uint64_t n2,
                                   int flags, uint64_t consumed[2], void *stream) {
  const int final_piece = flags & SCALCE_APPEND_FINAL;
  if (!b || !consumed || (n1 && !d_text1) || (b->nm == 2 && n2 && !d_text2)) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  if (b->tok_open) { set_err(c, "a tokenization is still open"); return SCALCE_ERR_ARG; }
  if (!b->appending) { batch_restart(b); b->appending = true; }
  const uint8_t *text[2] = {d_text1, d_text2};
  const u64 nbytes[2] = {n1, b->ntext == 2 ? n2 : 0};
  int rc = ingest_piece(b, text, nbytes, final_piece != 0, consumed, s);
  if (rc) return rc;
  if (!(flags & SCALCE_APPEND_NO_QUALITY) && (rc = scalce_batch_quality(b, stream))) return rc;
  if (!(flags & SCALCE_APPEND_NO_TOKENIZE) && (rc = scalce_batch_tokenize(b, nullptr, stream))) return rc;
  return SCALCE_OK;
}

// ingest_piece's verdict on the shape of a text that arrived at scalce_batch_rewindow (lines that make no whole records, no
// trailing newline, mates with different numbers of records), under rewindow's name and with ingest_piece's own words behind it
static int not_whole_records(scalce_ctx *c, const char *which) {
  const std::string why = c->err;
  set_err(c, "rewindow: the %s text is not whole records: %s", which, why.c_str());
  return SCALCE_ERR_FORMAT;
}

// Sharded runs: the rows this rank holds change at both ends (rank boundaries move to spill-chunk boundaries, sharded.cpp) --
// rows [keep_first, keep_first + keep_rows) stay, the records of `front` go in front of them, those of `back` behind (FASTQ text,
// whole records, either may be empty).  Rounds 1-4 rebuilt the whole range from text: a second ingest and a second first walk of
// every row (+21 ms per 50 M-read shard).  Here the rows that stay stay: the run-wide row arrays and the first walk's tokens are
// swapped against a second set in the workspace, the new set takes [front | kept | back] -- only the moved records are ingested
// and walked, the kept rows are one device copy (rows, name cells, tokens: ~185 bytes per read); nothing at all is copied when
// only the back end moves.  Quality statistics are NOT touched: every record was counted by the rank that ingested it first.
// An error behind the argument checks leaves the batch between the two sets of row arrays: its rows are gone, the next reset /
// ingest starts it over.
extern "C" int scalce_batch_rewindow(scalce_batch *b, uint64_t keep_first, uint64_t keep_rows, const uint8_t *const front[2],
                                     const uint64_t front_bytes[2], const uint8_t *const back[2], const uint64_t back_bytes[2], void *stream) {
  if (!b || !front || !back || !front_bytes || !back_bytes || keep_first + keep_rows > b->N || b->il || b->vl || b->keep_comments || b->keep_bases || b->keep_plus) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  if (b->tok_open || b->tok_done) { set_err(c, "rewindow: the rows have been tokenized already"); return SCALCE_ERR_ARG; }
  scalce_workspace &w = *b->ws;
  const bool walked = b->walk_rows == b->N && w.walk_owner == b && b->N > 0;  // (scalce_batch_chunk_plan has been here)
  const bool have_front = front_bytes[0] != 0;
  uint64_t used[2];
  const u64 fb[2] = {front_bytes[0], b->nm == 2 ? front_bytes[1] : 0}, bb[2] = {back_bytes[0], b->nm == 2 ? back_bytes[1] : 0};
  u64 nfront = 0;
  b->S_rows = ~0ull;
  b->appending = true;
  // rows the new range may hold (a record is at least "@x", L bases, "+", L qualities and four newlines): the tokens of the
  // first walk are sized for it BEFORE the kept ones move -- growing the array later would lose them
  const u64 rows_bound = keep_rows + fb[0] / (2 * (u64)b->L[0] + 7) + bb[0] / (2 * (u64)b->L[0] + 7) + 8;
  if (!have_front && keep_first == 0) {
    b->N = keep_rows;  // only the back end moves: rows beyond keep_rows are dropped where they lie
    if (walked) {
      int rc = ensure_keep(b, w.tok_bucket, sizeof(u32) * (rows_bound + 1), sizeof(u32) * keep_rows, s);
      if (!rc) rc = ensure_keep(b, w.tok_pos, sizeof(u32) * (rows_bound + 1), sizeof(u32) * keep_rows, s);
      if (rc) return rc;
    }
  } else {
    // the row arrays change places with the workspace's second set; the new set is filled [front | kept | back]
    DBuf *cur[] = {&w.packed[0], &w.packed[1], &w.q[0], &w.q[1], &w.namelen, &w.namecell, &w.name_in_off, &w.tok_bucket, &w.tok_pos};
    DBuf *alt[] = {&w.alt_packed[0], &w.alt_packed[1], &w.alt_q[0], &w.alt_q[1], &w.alt_namelen, &w.alt_namecell, &w.alt_name_in_off,
                   &w.alt_tok_bucket, &w.alt_tok_pos};
    const size_t elem[] = {(size_t)b->stride[0], (size_t)b->stride[1], (size_t)b->qstride[0], (size_t)b->qstride[1], 1, 16, 8, 4, 4};
    for (size_t i = 0; i < sizeof(cur) / sizeof(cur[0]); i++) {
      if (!cur[i]->p) continue;             // (an array this batch does not use: mate 2, names, long names)
      const bool tok = cur[i] == &w.tok_bucket || cur[i] == &w.tok_pos;
      ENSURE(b, *alt[i], std::max<size_t>(cur[i]->cap, tok ? sizeof(u32) * (rows_bound + 1) : 0));  // same capacity: reserve_rows sees one row_cap for both sets
      std::swap(*cur[i], *alt[i]);
    }
    // (the long-name STORE stays: name_in_off holds absolute positions in it, and the names of the rows that leave are only lost space)
    const u64 names_used = b->names_in_used;
    b->N = b->base = b->NP = 0;
    if (have_front) {
      int rc = ingest_piece(b, front, fb, true, used, s);
      if (rc == SCALCE_ERR_FORMAT) return not_whole_records(c, "front");
      if (rc) return rc;
      if (used[0] != fb[0] || (b->nm == 2 && used[1] != fb[1])) { set_err(c, "rewindow: the front text is not whole records"); return SCALCE_ERR_FORMAT; }
    }
    nfront = b->N;
    { int rc = reserve_rows(b, nfront + keep_rows, nfront, s); if (rc) return rc; }
    if (keep_rows) {
      for (size_t i = 0; i < sizeof(cur) / sizeof(cur[0]); i++) {
        if (!cur[i]->p || !alt[i]->p) continue;
        const bool tok = cur[i] == &w.tok_bucket || cur[i] == &w.tok_pos;
        if (tok && !walked) continue;
        if (cur[i] == &w.name_in_off && !names_used) continue;
        HIP_TRY(c, hipMemcpyAsync(cur[i]->as<u8>() + nfront * elem[i], alt[i]->as<u8>() + keep_first * elem[i], keep_rows * elem[i],
                                  hipMemcpyDeviceToDevice, s));
      }
    }
    b->N = nfront + keep_rows;
    b->base = b->N; b->NP = 0;
    b->ingested[0] = true; b->ingested[1] = b->nm == 2;
  }
  const u64 nkept_end = b->N;
  if (bb[0]) {
    int rc = ingest_piece(b, back, bb, true, used, s);
    if (rc == SCALCE_ERR_FORMAT) return not_whole_records(c, "back");
    if (rc) return rc;
    if (used[0] != bb[0] || (b->nm == 2 && used[1] != bb[1])) { set_err(c, "rewindow: the back text is not whole records"); return SCALCE_ERR_FORMAT; }
  }
  // the first walk of the rows that came in (the kept rows keep theirs)
  if (walked && w.tok_bucket.cap >= sizeof(u32) * (b->N + 1) && w.tok_pos.cap >= sizeof(u32) * (b->N + 1)) {
    launch_walk(b, WALK_FIRST, 0, nfront, 0, s);
    launch_walk(b, WALK_FIRST, nkept_end, b->N - nkept_end, 0, s);
    b->walk_rows = b->N;
    w.walk_owner = b;
  } else {
    b->walk_rows = 0;  // (scalce_batch_tokenize_begin walks every row)
  }
  return SCALCE_OK;
}

// back to rows that lie back to back (before anything is ingested): callers that read q' in input order as one array
// (sharded runs), runs sized for most of HBM (lean)
static void unfuse(scalce_batch *b) {
  if (!b->fused || b->N) return;
  b->fused = false;
  b->qstride[0] = (u32)b->L[0];
}
extern "C" void scalce_batch_set_lean(scalce_batch *b, int lean) {
  if (!b) return;
  b->lean = lean != 0;
  if (b->lean) unfuse(b);
}
extern "C" int scalce_batch_set_keep_order(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  b->keep_order = on != 0;
  return SCALCE_OK;
}
// what follows the names becomes an output of the run (SCALCE_OUT_COMMENTS): before the first ingest or append of the run
extern "C" int scalce_batch_set_keep_comments(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (on && !b->p.use_names) { set_err(b->ctx, "nothing is kept for what follows a name that is not kept"); return SCALCE_ERR_ARG; }
  b->keep_comments = on != 0;
  return SCALCE_OK;
}
// (for the other translation units of the library: sharded.cpp, pipeline.cpp)
bool scalce_batch_keeps_comments(const scalce_batch *b) { return b && b->keep_comments; }
extern "C" int scalce_batch_comments_info(const scalce_batch *b, int mate, uint64_t *nbytes, uint32_t *longest) {
  if (!b || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  if (nbytes) *nbytes = b->keep_comments ? b->com_used[mate] : 0;
  if (longest) *longest = b->keep_comments ? b->com_longest[mate] : 0;
  return SCALCE_OK;
}
// the '+' lines become an output of the run (SCALCE_OUT_PLUS): before the first ingest or append of the run
extern "C" int scalce_batch_set_keep_plus(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (on && (b->lpr != 4 || b->nq)) { set_err(b->ctx, "records without a '+' line (fasta, no_qualities) have none to keep"); return SCALCE_ERR_ARG; }
  if (on && b->code_in_place) { set_err(b->ctx, "a batch coded in place is run again from its text: the store would take its '+' lines twice"); return SCALCE_ERR_ARG; }
  if (b->N || b->appending || b->ingested[0]) { set_err(b->ctx, "keep-plus is set before the first ingest or append of a run"); return SCALCE_ERR_ARG; }
  b->keep_plus = on != 0;
  return SCALCE_OK;
}
// (for the other translation units of the library: sharded.cpp, pipeline.cpp)
bool scalce_batch_keeps_plus(const scalce_batch *b) { return b && b->keep_plus; }
extern "C" int scalce_batch_plus_info(const scalce_batch *b, int mate, uint64_t *nbytes, uint32_t *longest, uint64_t *repeats, uint64_t *literals) {
  if (!b || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  if (nbytes) *nbytes = b->keep_plus ? b->plus_used[mate] : 0;
  if (longest) *longest = b->keep_plus ? b->plus_longest[mate] : 0;
  if (repeats) *repeats = b->keep_plus ? b->plus_repeats[mate] : 0;
  if (literals) *literals = b->keep_plus ? b->plus_literals[mate] : 0;
  return SCALCE_OK;
}
// the letters and qualities the archive does not keep become an output of the run (SCALCE_OUT_EXCEPTIONS): before the first
// ingest or append of the run
extern "C" int scalce_batch_set_keep_bases(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (b->N || b->appending || b->ingested[0]) { set_err(b->ctx, "keep-bases is set before the first ingest or append of a run"); return SCALCE_ERR_ARG; }
  b->keep_bases = on != 0;
  return SCALCE_OK;
}
// (for the other translation units of the library: sharded.cpp, pipeline.cpp)
bool scalce_batch_keeps_bases(const scalce_batch *b) { return b && b->keep_bases; }
extern "C" int scalce_batch_exceptions_info(const scalce_batch *b, int mate, uint64_t *entries, uint64_t *records_with_one) {
  if (!b || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  if (entries) *entries = b->keep_bases ? b->exc_used[mate] : 0;
  if (records_with_one) *records_with_one = b->keep_bases ? b->exc_rows[mate] : 0;
  return SCALCE_OK;
}
extern "C" uint64_t scalce_batch_reruns(const scalce_batch *b) { return b ? b->reruns : 0; }
extern "C" int scalce_batch_coder_round(const scalce_batch *b) { return b ? b->ac_round_launched : 0; }
extern "C" int scalce_batch_set_code_in_place(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (on && (b->p.no_ac || b->lean || b->vl)) return SCALCE_ERR_ARG;  // (variable-length: a rerun would read the caller's text, not the padded one)
  if (on && b->keep_plus) return SCALCE_ERR_ARG;                       // (the rerun would append the text's '+' lines to the store again)
  b->code_in_place = on != 0;
  return SCALCE_OK;
}
extern "C" int scalce_batch_set_stream_scratch(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (on && (b->p.no_ac || b->lean)) return SCALCE_ERR_ARG;  // -A: the stream IS the output (compress.cpp:389-390)
  b->qs_in_ws = on != 0;
  return SCALCE_OK;
}
extern "C" int scalce_batch_set_fused_rows(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  if (!on) unfuse(b);
  return (on != 0) == b->fused ? SCALCE_OK : SCALCE_ERR_ARG;
}

// ---- stage 1: quality statistics -------------------------------------------------------------------
// what the last piece_unpack_t did for `mate`: {kernel, slow, line index built, long-name bytes} -- the host's own branches,
// nothing is read back
extern "C" int scalce_batch_ingest_plan(const scalce_batch *b, int mate, uint32_t out[4]) {
  if (!b || !out || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = b->ingest_plan[mate][i];
  return SCALCE_OK;
}

// where a mate's symbol range came from (scalce_batch_quality_plan, scalce_hip.h)
enum QualitySource : u32 { QSRC_NONE = 0, QSRC_TILES = 1, QSRC_ROWS = 2, QSRC_WHOLE = 3 };
extern "C" int scalce_batch_quality(scalce_batch *b, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  b->quality_source[0] = b->quality_source[1] = QSRC_NONE;
  if (b->nq) return SCALCE_OK;  // -Q / -f: no qualities, no statistics (compress.cpp:689,697) -- nothing is launched
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_QUALITY, s);
  for (int m = 0; m < b->nm; m++) {
    if (!b->ingested[m]) { set_err(c, "ingest mate %d first", m + 1); return SCALCE_ERR_ARG; }
    if (b->base == 0) {  // counters run over all pieces of the batch
      HIP_TRY(c, hipMemsetAsync(b->freq4[m].p, 0, sizeof(u64) * 512000, s));
      b->tri_expected[m] = 0;
    }
    if (b->p.no_ac) continue;  // statistics are skipped under -A (qualities.cpp:185)
    const u64 n = b->NP * (u64)b->L[m], before = b->base * (u64)b->L[m];
    if (!n) continue;
    const u8 *q = w.q[m].as<u8>() + b->base * (u64)b->qstride[m];  // the piece's first row
    u32 *minmax = b->d_scr->minmax;  // smallest / largest symbol of the piece
    HIP_TRY(c, hipMemsetAsync(minmax, 0xFF, sizeof(u32), s));
    HIP_TRY(c, hipMemsetAsync(minmax + 1, 0, sizeof(u32), s));
    // the ingest kernel left the range of every tile of the piece's text -- in the WORKSPACE: if another batch that shares it
    // has ingested since, the ranges are that batch's, and the piece's own q' rows are scanned instead
    if (b->mm_valid[m] && w.tile_mm_owner[m] == b) {
      const u32 nt = cdiv(b->text_bytes[m], ING_TILE);
      LAUNCH(tile_minmax_reduce_k, cdiv(nt, 256 * 16) ? cdiv(nt, 256 * 16) : 1, 256, 0, s, w.tile_mm[m].as<u16>(), nt, minmax);
      b->quality_source[m] = QSRC_TILES;
    } else if (b->qstride[m] != (u32)b->L[m]) {
      // (fused rows and no tile ranges -- another batch of the workspace has ingested since: the whole alphabet, more passes)
      static const u32 whole[2] = {0u, 79u};
      HIP_TRY(c, hipMemcpyAsync(minmax, whole, sizeof whole, hipMemcpyHostToDevice, s));
      b->quality_source[m] = QSRC_WHOLE;
    } else {
      LAUNCH(sym_range_k, 2048, 256, 0, s, q, n, minmax);
      b->quality_source[m] = QSRC_ROWS;
    }
    u32 *prev = b->d_scr->prev[m];  // the two symbols in front of this piece
    LAUNCH(tri_prev_k, 1, 1, 0, s, w.q[m].as<u8>(), (u32)b->L[m], b->qstride[m], before, b->p.qprev[m][0], b->p.qprev[m][1], prev);
    u32 *range = b->d_scr->range[m];  // {lo, A, all symbols inside}: span of the symbols that occur
    LAUNCH(tri_range_k, 1, 1, 0, s, minmax, prev, range);
    unsigned long long *tiles = b->d_scr->tri_tiles;  // one tile counter per pass
    HIP_TRY(c, hipMemsetAsync(tiles, 0, sizeof b->d_scr->tri_tiles, s));
    for (u32 pass = 0; pass < 3; pass++)  // pass 0, pass 1, and whatever a wide alphabet needs behind them in one launch
      LAUNCH(trigram_pass_k, b->tri_grid, TRI_THREADS, 0, s, q, n, prev, pass, pass < 2 ? pass + 1 : (u32)TRI_MAX_PASSES, range, b->freq4[m].as<u64>(), tiles,
             (u32)b->L[m], b->qstride[m]);
    {  // one count per symbol with two predecessors (the run's first two have them only when the caller passed qprev)
      const bool p0 = b->p.qprev[m][0] < 80, p1 = b->p.qprev[m][1] < 80;
      const u64 carried = p1 ? (p0 ? 2 : 1) : 0;
      const u64 have = carried + before >= 2 ? 2 : carried + before;
      b->tri_expected[m] += n > 2 - have ? n - (2 - have) : 0;
      BatchScratch::TriCheck *chk = &b->d_scr->tri_check[m];
      HIP_TRY(c, hipMemsetAsync(chk, 0, sizeof *chk, s));
      LAUNCH(tri_check_k, 64, 256, 0, s, b->freq4[m].as<u64>(), b->tri_expected[m], &chk->acc, &chk->done, b->d_err);
    }
  }
  return SCALCE_OK;
}

// what the last scalce_batch_quality did for `mate`: {source, lo, A, inside} -- the branch the host took and what tri_range_k
// left in range[mate].  Waits for the device and reads back: for tests.
extern "C" int scalce_batch_quality_plan(const scalce_batch *b, int mate, uint32_t out[4]) {
  if (!b || !out || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  out[0] = b->quality_source[mate];
  out[1] = out[2] = out[3] = 0;
  if (out[0] == QSRC_NONE) return SCALCE_OK;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(out + 1, b->d_scr->range[mate], 3 * sizeof(u32), hipMemcpyDeviceToHost));
  return SCALCE_OK;
}
