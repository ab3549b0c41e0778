// host_order_emit.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): stages 3 and 4: spill chunks, radix passes on (key, read) pairs, run sorts; records, names, the reordered stream
// ---- stage 3: order ----------------------------------------------------------------------------------
extern "C" int scalce_batch_order(scalce_batch *b, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_ORDER, s);
  const u64 N = b->N;
  const u32 nb1 = (u32)c->A.n_buckets + 1;
  ENSURE(b, w.perm_a, sizeof(u32) * (N + 2));
  ENSURE(b, w.perm_b, sizeof(u32) * (N + 2));
  ENSURE(b, w.hist, sizeof(u32) * radix_hist_elems(N));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(radix_hist_elems(N)) + scan_ws_elems(N + 1) + 1024));
  b->perm = w.perm_a.as<u32>();
  b->sorted_keys = nullptr;
  b->nchunks = 1;
  if (!N) return SCALCE_OK;
  u32 *ws32 = w.scan_ws.as<u32>();
  // spill chunks: given explicitly (sharded runs: one chunk per shard) or by the -B rule
  if (!b->explicit_chunks.empty()) {
    const u32 nc = (u32)b->explicit_chunks.size();
    ENSURE(b, w.chunk, sizeof(u32) * (N + 2));
    ENSURE(b, w.chunk_start, sizeof(u64) * (nc + 2));
    std::vector<u64> cs(b->explicit_chunks.begin(), b->explicit_chunks.end());
    cs.push_back(N);
    HIP_TRY(c, hipMemcpyAsync(w.chunk_start.p, cs.data(), sizeof(u64) * cs.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(&b->d_scr->nchunks, &nc, sizeof(u32), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    b->nchunks = nc;
    if (nc > 1) LAUNCH(chunk_assign_k, cdiv(N, 256), 256, 0, s, N, w.chunk_start.as<u64>(), &b->d_scr->nchunks, w.chunk.as<u32>());
  } else if (b->p.bucket_set_size) {
    ENSURE(b, w.S, sizeof(u64) * (N + 2));
    b->S_rows = ~0ull;
    ENSURE(b, w.chunk, sizeof(u32) * (N + 2));
    // No cap on the cuts (the reference has none, compress.cpp:708-715).  A chunk holds at least one record and every chunk but
    // the last at least -B bytes, and no record is larger than rec_max: that bounds the chunks from the host, without a read-back.
    const u64 rec_max = 1 + 255 + 40 + (u64)b->szr[0] + (u64)b->L[0] + (b->p.paired ? (u64)b->szr[1] + (u64)b->L[1] : 0);
    u64 chunks_max = N * rec_max / (u64)b->p.bucket_set_size + 1;
    if (chunks_max > N) chunks_max = N;
    const u32 max_chunks = (u32)chunks_max + 1;  // (chunk_bounds_k makes fewer cuts than this)
    ENSURE(b, w.chunk_start, sizeof(u64) * (chunks_max + 2));
    // (-Q / -f: rd.sz holds no quality bytes, compress.cpp:689-702 -- the cuts fall elsewhere than with qualities)
    RecSize rs{w.bucket.as<u32>(), c->d_bucket_level.as<u32>(), w.namelen.as<u8>(), b->L[0], b->L[1], b->p.paired, b->p.use_names, !b->nq};
    u64 *S = w.S.as<u64>();
    exclusive_scan<u64>(rs, N, StoreTo<u64>{S}, w.scan_ws.as<u64>(), S + N, s);
    LAUNCH(chunk_bounds_k, 1, 1, 0, s, S, N, (u64)b->p.bucket_set_size, max_chunks, w.chunk_start.as<u64>(), &b->d_scr->nchunks);
    int rc = read_u32(b, &b->d_scr->nchunks, &b->nchunks, 1, s);
    if (rc) return rc;
    if (b->nchunks == CHUNKS_OVERFLOW) {
      b->nchunks = 1;
      set_err(c, "the -B rule cuts more than the %llu spill chunks the order stage allowed for", (unsigned long long)chunks_max);
      return SCALCE_ERR_CAPACITY;
    }
    if (b->nchunks > 1)
      LAUNCH(chunk_assign_k, cdiv(N, 256), 256, 0, s, N, w.chunk_start.as<u64>(), &b->d_scr->nchunks, w.chunk.as<u32>());
  }
  const u32 *src = nullptr;
  u32 *dst = w.perm_a.as<u32>(), *alt = w.perm_b.as<u32>();
  auto flip = [&]() { src = dst; u32 *t = dst; dst = alt; alt = t; };
  const int ndig = (b->L[0] + 3) / 4;
  const bool two_phase = getenv("SCALCE_ORDER_SINGLE_PHASE") == nullptr;  // test hook: all digits in one go
  const int ndig1 = two_phase ? (ndig < PREFIX_DIGITS ? ndig : PREFIX_DIGITS) : ndig;
  const u32 *chunk_or_null = b->nchunks > 1 ? w.chunk.as<u32>() : nullptr;
  int bits = 1;
  while ((1u << bits) < nb1 && bits < 31) bits++;
  int cbits = 0;
  while (b->nchunks > 1 && (1ull << cbits) < b->nchunks) cbits++;
  // phase 1 on (key, read) pairs when bucket | chunk | 32 prefix bits fit 64 bits (always, short of a million cores
  // together with more than 4096 chunks): every pass then reads and writes sequentially.  The index-only passes below
  // gather a digit through the index in every pass: 8 GB of sector fetches per pass at 50 M reads, and the scattered
  // accesses are what slows a coder launch running beside the order stage most (DESIGN_HISTORY.md).
  const bool by_pairs = two_phase && PREFIX_BITS + cbits + bits <= 64;
  u64 *sorted_keys = nullptr;
  const u32 end_bits = (16 + PREFIX_BITS + cbits + bits <= 64) ? 16u : 0u;
  if (by_pairs) {
    ENSURE(b, w.key_a, sizeof(u64) * (N + 2));
    ENSURE(b, w.key_b, sizeof(u64) * (N + 2));
    u64 *ka = w.key_a.as<u64>(), *kb = w.key_b.as<u64>();
    LAUNCH(order_keys_k, cdiv(N, 256), 256, 0, s, (u32)N, w.bucket.as<u32>(), chunk_or_null, (u32)cbits, w.packed[0].as<u8>(),
           w.endv.as<u16>(), b->L[0], b->stride[0], ndig1, end_bits, ka);
    for (int sh = (int)end_bits; sh < (int)end_bits + PREFIX_BITS + cbits + bits; sh += 8) {
      radix_pass_kv(ka, src, kb, dst, (u32)N, (u32)sh, w.hist.as<u32>(), ws32, s);
      flip();
      u64 *t = ka; ka = kb; kb = t;
    }
    sorted_keys = ka;
    b->sorted_keys = ka;
    b->key_end_bits = end_bits;
    b->key_bucket_shift = end_bits + PREFIX_BITS + (u32)cbits;
    b->key_bucket_mask = (1u << bits) - 1;
  } else {
    // phase 1: first ndig1 key digits (least significant first), then chunk, then bucket
    for (int d = ndig1 - 1; d >= 0; d--) {
      radix_pass(src, dst, (u32)N, KeyDigit{w.packed[0].as<u8>(), w.endv.as<u16>(), b->L[0], b->stride[0], d}, w.hist.as<u32>(),
                 ws32, s);
      flip();
    }
    if (b->nchunks > 1)
      for (int sh = 0; (1ull << sh) < b->nchunks; sh += 8) {
        radix_pass(src, dst, (u32)N, DigitOfArray{w.chunk.as<u32>(), sh}, w.hist.as<u32>(), ws32, s);
        flip();
      }
    for (int sh = 0; sh < bits; sh += 8) {
      radix_pass(src, dst, (u32)N, DigitOfArray{w.bucket.as<u32>(), sh}, w.hist.as<u32>(), ws32, s);
      flip();
    }
  }
  u32 *perm1 = const_cast<u32 *>(src);
  b->order_run_members = 0;
  b->order_radix_fallback = 0;
  if (ndig1 < ndig) {
    // phase 2: records that still tie on (bucket, chunk, prefix) are sorted on the remaining digits, run by run
    ENSURE(b, w.run_head, N + 64);
    ENSURE(b, w.run_hcount, sizeof(u32) * (N + 2));
    ENSURE(b, w.run_rank, sizeof(u32) * (N + 2));
    ENSURE(b, w.runid, sizeof(u32) * (N + 2));
    RunArgs ra{(u32)N, perm1, w.bucket.as<u32>(), chunk_or_null, w.packed[0].as<u8>(), w.endv.as<u16>(), b->L[0], b->stride[0], ndig1};
    u8 *head = w.run_head.as<u8>();
    if (sorted_keys) LAUNCH(run_heads_keys_k, cdiv(N, 256), 256, 0, s, (u32)N, sorted_keys, end_bits, head);
    else LAUNCH(run_heads_k, cdiv(N, 256), 256, 0, s, ra, head);
    exclusive_scan<u32>(LoadAs<u8, u32>{head}, N, StoreTo<u32>{w.run_hcount.as<u32>()}, ws32, (u32 *)nullptr, s);
    exclusive_scan<u32>(RunMember{head, (u32)N}, N, StoreTo<u32>{w.run_rank.as<u32>()}, ws32, &b->d_scr->run_members, s);
    u32 M = 0;
    { int rc = read_u32(b, &b->d_scr->run_members, &M, 1, s); if (rc) return rc; }
    b->order_run_members = M;
    if (M) {
      ENSURE(b, w.run_items_a, sizeof(u32) * (M + 2));
      ENSURE(b, w.run_items_b, sizeof(u32) * (M + 2));
      ENSURE(b, w.run_pos, sizeof(u32) * (M + 2));
      LAUNCH(run_compact_k, cdiv(N, 256), 256, 0, s, (u32)N, head, w.run_rank.as<u32>(), w.run_hcount.as<u32>(), perm1,
             w.run_items_a.as<u32>(), w.run_pos.as<u32>(), w.runid.as<u32>());
      bool small_done = false;
      {  // runs of up to 32 members are sorted where they stand (run_small_sort_k)
        u32 *any_large = &b->d_scr->any_large;
        HIP_TRY(c, hipMemsetAsync(any_large, 0, sizeof(u32), s));
        LAUNCH(run_small_sort_k, cdiv(M, 256), 256, 0, s, M, w.run_pos.as<u32>(), head, (u32)N, perm1, sorted_keys, end_bits,
               w.packed[0].as<u8>(), w.endv.as<u16>(), b->L[0], b->stride[0], ndig1, ndig, any_large);
        u32 large = 0;
        { int rc = read_u32(b, any_large, &large, 1, s); if (rc) return rc; }
        b->order_radix_fallback = large;
        small_done = large == 0;
      }
      if (!small_done) {
      const u32 *rs = w.run_items_a.as<u32>();
      u32 *rd = w.run_items_b.as<u32>(), *ralt = w.run_items_a.as<u32>();
      auto rflip = [&]() { rs = rd; u32 *t = rd; rd = ralt; ralt = t; };
      for (int d = ndig - 1; d >= ndig1; d--) {
        radix_pass(rs, rd, M, KeyDigit{w.packed[0].as<u8>(), w.endv.as<u16>(), b->L[0], b->stride[0], d}, w.hist.as<u32>(), ws32, s);
        rflip();
      }
      int rbits = 1;
      while ((1ull << rbits) <= N && rbits < 32) rbits++;  // run ids are at most N
      for (int sh = 0; sh < rbits; sh += 8) {
        radix_pass(rs, rd, M, DigitOfArray{w.runid.as<u32>(), sh}, w.hist.as<u32>(), ws32, s);
        rflip();
      }
      LAUNCH(run_scatter_k, cdiv(M, 256), 256, 0, s, M, rs, w.run_pos.as<u32>(), perm1, sorted_keys, end_bits, w.endv.as<u16>());
      }
    }
  }
  b->perm = perm1;
  // variable-length runs: L - length in output order (mate 2 follows mate 1's order, like its reads)
  for (int m = 0; m < b->nm && b->vl; m++) {
    ENSURE(b, b->out_lengths[m], sizeof(u16) * (N + 64));
    LAUNCH(gather_padlen_k, cdiv(N, 256), 256, 0, s, N, b->perm, w.padlen[m].as<u16>(), b->out_lengths[m].as<u16>());
  }
  return SCALCE_OK;
}

// ---- stage 4: emit -----------------------------------------------------------------------------------
extern "C" int scalce_batch_emit(scalce_batch *b, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  scalce_workspace &w = *b->ws;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  StageTimer tm(b, ST_EMIT, s);
  const u64 N = b->N;
  const u32 nb1 = (u32)c->A.n_buckets + 1;
  ENSURE(b, w.bucket_first, sizeof(u64) * (nb1 + 2));
  ENSURE(b, w.bucket_off, sizeof(u64) * (nb1 + 2));
  ENSURE(b, w.scan_ws, sizeof(u64) * (scan_ws_elems(nb1) + scan_ws_elems(N + 1) + 1024));
  u64 *ws = w.scan_ws.as<u64>();
  u64 *counts = b->counts_total.as<u64>();  // reads per bucket over every piece of the batch
  if (!counts) { set_err(c, "tokenize first"); return SCALCE_ERR_ARG; }
  exclusive_scan<u64>(LoadAs<u64, u64>{counts}, nb1, StoreTo<u64>{w.bucket_first.as<u64>()}, ws, &b->d_scr->emit.reads, s);
  exclusive_scan<u64>(BucketBytes{counts, c->d_bucket_level.as<u32>(), b->L[0], b->sz_meta}, nb1, StoreTo<u64>{w.bucket_off.as<u64>()}, ws,
                      &b->d_scr->emit.read_bytes, s);
  if (b->p.use_names) {
    ENSURE(b, w.name_off, sizeof(u64) * (N + 2));
    ENSURE(b, w.outlen, N + 64);
    // the name cells are gathered through the permutation ONCE, into output order: their first byte is the length the scan
    // wants, and emit_names_sorted_k then reads them in sequence (name_outlen_k + emit_names_k gathered twice)
    // (not in lean mode: a run sized for most of HBM has no 16 bytes per read to spare, and allocating and releasing
    //  3 GB costs more than the second gather)
    const bool cells = w.namecell.p != nullptr && !b->lean;
    b->names_from_sorted_cells = cells;
    if (cells) ENSURE(b, w.cell_sorted, 16 * (N + 4));
    if (N && cells) LAUNCH(name_cells_sorted_k, cdiv(N, 256), 256, 0, s, N, b->perm, w.namecell.as<u8>(), w.cell_sorted.as<u8>(), w.outlen.as<u8>());
    else if (N) LAUNCH(name_outlen_k, cdiv(N, 256), 256, 0, s, N, b->perm, w.namelen.as<u8>(), w.outlen.as<u8>());
    exclusive_scan<u64>(NameLenSeq{w.outlen.as<u8>()}, N, StoreTo<u64>{w.name_off.as<u64>()}, ws, &b->d_scr->emit.name_bytes, s);
    ENSURE(b, b->bucket_name_bytes, sizeof(u64) * (nb1 + 1));
    LAUNCH(bucket_name_bytes_k, cdiv(nb1, 256), 256, 0, s, nb1, w.bucket_first.as<u64>(), counts, w.name_off.as<u64>(), &b->d_scr->emit.name_bytes, N,
           b->bucket_name_bytes.as<u64>());
  }
  BatchScratch::EmitTotals h = {0, 0, 0};
  { int rc = read_words(b, &b->d_scr->emit, &h, sizeof h / 4, s); if (rc) return rc; }
  b->out_reads_bytes[0] = h.read_bytes;
  b->out_names_bytes = b->p.use_names ? h.name_bytes : 0;
  ENSURE(b, b->out_reads[0], h.read_bytes + 64);
  ENSURE(b, b->out_names, b->out_names_bytes + 64);
  if (N) {
    EmitArgs a;
    a.nrec = N; a.perm = b->perm; a.bucket = w.bucket.as<u32>(); a.end = w.endv.as<u16>(); a.packed = w.packed[0].as<u8>();
    a.L = b->L[0]; a.stride = b->stride[0]; a.sz_meta = b->sz_meta; a.bucket_level = c->d_bucket_level.as<u32>();
    a.bucket_pattern = c->d_bucket_pattern.as<int32_t>(); a.bucket_first = w.bucket_first.as<u64>(); a.bucket_off = w.bucket_off.as<u64>();
    a.counts = counts; a.out = b->out_reads[0].as<u8>();
    a.keys = b->sorted_keys; a.key_bucket_shift = b->key_bucket_shift; a.key_bucket_mask = b->key_bucket_mask;
    a.key_end_bits = b->key_end_bits;
    a.pwords = 0; a.frow = nullptr; a.cells_sorted = a.outlen = a.qs = nullptr; a.cell_off = a.qunits = 0; a.qmagic = a.rmagic = a.lmagic = 0;
    if (b->fused) {
      // One row per read: the workgroup that assembles a record's bases also moves its q' into the reordered stream -- both
      // lie in ONE row of the ingest stage's making (128 bytes = one aligned line at 100 bp), fetched whole into LDS with every
      // thread's loads in flight at once.  One random line per record instead of three (packed row + q' row for
      // gather_rows_k, each paying its own).
      ENSURE(b, b->qs(0), (size_t)b->L[0] * N + 64 + AC_INPLACE_PAD);
      a.frow = w.q[0].as<u8>(); a.stride = (int)b->qstride[0]; a.cell_off = b->row_cell_off; a.pwords = (int)b->row_pwords;
      a.packed = a.frow + b->row_cell_off;
      a.qunits = ((u32)b->L[0] + 15) / 16;
      a.qmagic = ((1ull << 32) + a.qunits - 1) / a.qunits;
      a.rmagic = ((1ull << 32) + (b->qstride[0] >> 4) - 1) / (b->qstride[0] >> 4);
      a.lmagic = ((1ull << 32) + (u32)b->L[0] - 1) / (u32)b->L[0];
      a.qs = b->qs(0).as<u8>();
      const size_t rows_lds = 256 * (size_t)b->qstride[0];
      if (rows_lds > 32 * 1024)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(emit_reads_k<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_lds));
      LAUNCH(emit_reads_k<true>, cdiv(N, 256), 256, rows_lds, s, a);
    } else
    LAUNCH(emit_reads_k<false>, cdiv(N, 256), 256, 0, s, a);
    if (b->p.use_names && b->names_from_sorted_cells)
      LAUNCH(emit_names_sorted_k, cdiv(N, 256), 256, 0, s, N, b->perm, w.cell_sorted.as<u8>(), w.name_in_off.as<u64>(),
             w.names_in.as<u8>(), w.name_off.as<u64>(), b->out_names.as<u8>());
    else if (b->p.use_names)
      LAUNCH(emit_names_k, cdiv(N, 256), 256, 0, s, N, b->perm, w.namecell.as<u8>(), w.name_in_off.as<u64>(),
             w.names_in.as<u8>(), w.name_off.as<u64>(), b->out_names.as<u8>());
    for (int m = 0; m < b->nm && !b->nq; m++) {  // (-Q / -f: no quality stream)
      const u32 width = (u32)b->L[m];
      if (m == 0 && b->fused) continue;  // (emit_reads_k<true> has done it)
      ENSURE(b, b->qs(m), (size_t)width * N + 64 + AC_INPLACE_PAD);
      LAUNCH(gather_rows_k, gather_grid(N, width), 256, 0, s, N, b->perm, w.q[m].as<u8>(), (u64)b->qstride[m], width, b->qs(m).as<u8>());
      if (b->lean) {
        // q' in input order is dead once its reordered copy exists.  Mate 1's buffer becomes mate 2's reordered stream (an
        // allocation and a release of tens of GB each cost a good part of a second), the last one is released.
        HIP_TRY(c, hipStreamSynchronize(s));
        if (m == 0 && b->nm == 2 && !b->qs(1).p && w.q[0].cap >= (size_t)b->L[1] * N + 64) {
          b->qs(1) = std::move(w.q[0]);
        } else {
          w.q[m].release();
        }
      }
    }
    if (b->nm == 2) {  // mate 2: bare packed reads in the same order (compress.cpp:380-383 with fR = file 4)
      const u32 width = (u32)b->szr[1];
      b->out_reads_bytes[1] = N * width;
      ENSURE(b, b->out_reads[1], N * width + 64);
      LAUNCH(gather_rows_k, gather_grid(N, width), 256, 0, s, N, b->perm, w.packed[1].as<u8>(), (u64)b->stride[1], width,
             b->out_reads[1].as<u8>());
    }
  } else if (b->nm == 2) b->out_reads_bytes[1] = 0;
  // what follows the names, in archive order: output record k is input record perm[k] of the mate's store -- the permute of the
  // order restore (scalce_records_permute), with the scan of the rows' entry sizes for the store's offsets
  for (int m = 0; m < b->nm && b->keep_comments; m++) {
    b->out_comments_bytes[m] = N ? b->com_used[m] : 0;
    if (!N) continue;
    ENSURE(b, b->com_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->com_out_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->com_ws, (size_t)scalce_records_permute_ws_bytes(N));
    ENSURE(b, b->out_comments[m], (size_t)b->com_used[m] + 64);
    u64 *off = b->com_off.as<u64>();
    exclusive_scan<u64>(CommentSize{b->comlen[m].as<u16>()}, N, StoreTo<u64>{off}, b->com_ws.as<u64>(), off + N, s);
    int rc = scalce_records_permute(c, b->com_in[m].as<u8>(), b->com_off.as<uint64_t>(), N, b->com_used[m], b->perm, b->out_comments[m].as<u8>(), b->com_used[m],
                                    b->com_out_off.as<uint64_t>(), b->com_ws.p, s);
    if (rc) return rc;
    if (b->lean) {  // the input-order store is dead once the gathered stream exists
      HIP_TRY(c, hipStreamSynchronize(s));
      b->com_in[m].release();
      b->comlen[m].release();
    }
  }
  // the '+' lines, in archive order: the same gather over the plus store; the classes are counted for the log on the way
  for (int m = 0; m < b->nm && b->keep_plus; m++) {
    b->out_plus_bytes[m] = N ? b->plus_used[m] : 0;
    if (!N) continue;
    ENSURE(b, b->com_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->com_out_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->com_ws, (size_t)scalce_records_permute_ws_bytes(N));
    ENSURE(b, b->out_plus[m], (size_t)b->plus_used[m] + 64);
    u64 *off = b->com_off.as<u64>();
    const u16 *len = b->pluslen[m].as<u16>();
    HIP_TRY(c, hipMemsetAsync(b->d_scr->plus_classes[m], 0, 2 * sizeof(u32), s));
    LAUNCH(plus_count_k, cdiv(N, 256), 256, 0, s, N, len, b->d_scr->plus_classes[m]);
    exclusive_scan<u64>(CommentSize{len}, N, StoreTo<u64>{off}, b->com_ws.as<u64>(), off + N, s);
    int rc = scalce_records_permute(c, b->plus_in[m].as<u8>(), b->com_off.as<uint64_t>(), N, b->plus_used[m], b->perm, b->out_plus[m].as<u8>(), b->plus_used[m],
                                    b->com_out_off.as<uint64_t>(), b->com_ws.p, s);
    if (rc) return rc;
    u32 cls[2] = {0, 0};
    { int rc2 = read_u32(b, b->d_scr->plus_classes[m], cls, 2, s); if (rc2) return rc2; }
    b->plus_repeats[m] = cls[0]; b->plus_literals[m] = cls[1];
    if (b->lean) {  // the input-order store is dead once the gathered stream exists
      HIP_TRY(c, hipStreamSynchronize(s));
      b->plus_in[m].release();
      b->pluslen[m].release();
    }
  }
  // the exceptions, in archive order: the entries of output record k are those of input record perm[k], with k stamped in --
  // two scans of the rows' counts (input order for the store's offsets, permuted for the stream's) and one gather
  if (b->keep_bases && N >= EXC_MAX_RECORDS) {  // (36 bits of an entry name its record)
    set_err(c, "(ERROR) --keep-bases: %llu records are more than the 2^36 - 1 an exception stream can name", (unsigned long long)N);
    return SCALCE_ERR_CAPACITY;
  }
  for (int m = 0; m < b->nm && b->keep_bases; m++) {
    b->out_exc_entries[m] = N ? b->exc_used[m] : 0;
    if (!N || !b->exc_used[m]) {
      if (b->lean) { HIP_TRY(c, hipStreamSynchronize(s)); b->exc_in[m].release(); }  // (a store an earlier run of the batch left)
      continue;
    }
    ENSURE(b, b->exc_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->exc_out_off, sizeof(u64) * (N + 8));
    ENSURE(b, b->exc_ws, sizeof(u64) * (scan_ws_elems(N) + 64));
    ENSURE(b, b->out_exc[m], sizeof(u64) * (b->exc_used[m] + 8));
    const u16 *cnt = b->exc_cnt[m].as<u16>();
    u64 *off = b->exc_off.as<u64>(), *out_off = b->exc_out_off.as<u64>();
    exclusive_scan<u64>(ExcCount{cnt}, N, StoreTo<u64>{off}, b->exc_ws.as<u64>(), off + N, s);
    exclusive_scan<u64>(ExcCountPermuted{cnt, b->perm}, N, StoreTo<u64>{out_off}, b->exc_ws.as<u64>(), out_off + N, s);
    LAUNCH(exc_gather_k, cdiv(N, 256), 256, 0, s, N, b->perm, cnt, off, b->exc_in[m].as<u64>(), out_off, b->out_exc[m].as<u64>());
    if (b->lean) {  // the input-order store is dead once the gathered stream exists
      HIP_TRY(c, hipStreamSynchronize(s));
      b->exc_in[m].release();
    }
  }
  if (b->lean && b->keep_bases) {
    HIP_TRY(c, hipStreamSynchronize(s));
    for (int m = 0; m < b->nm; m++) b->exc_cnt[m].release();
    b->exc_off.release(); b->exc_out_off.release(); b->exc_ws.release(); b->exc_piece_off.release();
  }
  if (b->lean && (b->keep_comments || b->keep_plus)) { b->com_off.release(); b->com_out_off.release(); b->com_ws.release(); b->com_piece_off.release(); }
  if (b->lean) {  // nothing behind this stage reads the rows, the tokens or the sort scratch
    HIP_TRY(c, hipStreamSynchronize(s));
    DBuf *dead[] = {&w.packed[0], &w.packed[1], &w.namecell, &w.names_in, &w.name_in_off, &w.name_off, &w.outlen, &w.cell_sorted,
                    &w.line_end[0], &w.line_end[1], &w.tile[0], &w.tile[1], &w.tok_bucket, &w.tok_pos, &w.tie_index,
                    &w.tie_read, &w.tie_off, &w.tie_ncand, &w.cand_bucket, &w.cand_pos, &w.choice, &w.ev_off,
                    &w.ev_sorted, &w.ev_tmp, &w.ev_place, &w.chosen, &w.G, &w.cand_place,
                    &w.bucket, &w.endv, &w.tokens, &w.chunk, &w.chunk_start, &w.perm_a, &w.perm_b, &w.key_a, &w.key_b, &w.hist, &w.S,
                    &w.run_head, &w.run_hcount, &w.run_rank, &w.runid, &w.run_items_a, &w.run_items_b, &w.run_pos};
    // (keep_order: the permutation is an output of the run -- the half of the pair it lies in stays, and so does the pointer)
    const bool keep_perm = b->keep_order && b->perm;
    for (DBuf *d : dead) {
      if (keep_perm && d->p && (u8 *)b->perm >= d->as<u8>() && (u8 *)b->perm < d->as<u8>() + d->cap) continue;
      if (d->cap >= (256u << 20)) d->release();  // (the big ones; releasing dozens of small buffers only costs time)
    }
    if (!keep_perm) b->perm = nullptr;
    b->sorted_keys = nullptr;
    w.row_cap = 0;
  }
  return SCALCE_OK;
}
