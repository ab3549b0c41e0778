// host_api.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): whole-shard entry points, outputs, timers, small utilities, the coder self-test
extern "C" int scalce_batch_compress(scalce_batch *b, const uint8_t *t1, uint64_t n1, const uint8_t *t2, uint64_t n2, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  int rc;
  if ((rc = scalce_batch_ingest(b, 0, t1, n1, stream))) return rc;
  if (b->ntext == 2 && (rc = scalce_batch_ingest(b, 1, t2, n2, stream))) return rc;  // (-i: mate 0's text holds both)
  if ((rc = scalce_batch_quality(b, stream))) return rc;
  if ((rc = scalce_batch_tokenize(b, nullptr, stream))) return rc;
  if ((rc = scalce_batch_order(b, stream))) return rc;
  if ((rc = scalce_batch_emit(b, stream))) return rc;
  if ((rc = scalce_batch_entropy(b, nullptr, stream))) return rc;
  return SCALCE_OK;
}

// Every stage in front of the entropy coder (ingest .. emit) of a shard that is resident as text, on `stream` -- except the
// quality statistics, which the tokenizer forks onto the workspace's side stream beside the tie-break's window sweeps
// (quality_beside, host_tokenize.inc: ev_fork, then ev_side behind the statistics); `stream` waits for ev_side before it
// returns, so everything behind this call sees the statistics.  With stage times taken, or -A, they stay on `stream`.
extern "C" int scalce_batch_front(scalce_batch *b, const uint8_t *t1, uint64_t n1, const uint8_t *t2, uint64_t n2, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  int rc;
  if ((rc = scalce_batch_ingest(b, 0, t1, n1, stream))) return rc;
  if (b->ntext == 2 && (rc = scalce_batch_ingest(b, 1, t2, n2, stream))) return rc;  // (-i: mate 0's text holds both)
  // the quality statistics run beside the tie-break's sweeps (quality_beside, host_tokenize.inc) -- or here, when the
  // tokenizer never gets there (no tie reads, another tie-break path) or stage times are being taken
  b->quality_deferred = !b->timing && !b->p.no_ac && !b->nq;  // (-Q / -f: nothing to fork)
  if (!b->quality_deferred && (rc = scalce_batch_quality(b, stream))) return rc;
  rc = scalce_batch_tokenize(b, nullptr, stream);
  if (b->quality_deferred) {
    b->quality_deferred = false;
    if (!rc) rc = scalce_batch_quality(b, stream);
  }
  if (!rc) rc = scalce_batch_order(b, stream);
  if (!rc) rc = scalce_batch_emit(b, stream);
  if (b->side_busy) {  // (also on the way out of an error: the side stream must not run into the next shard's rows)
    b->side_busy = false;
    HIP_TRY(b->ctx, hipStreamWaitEvent((hipStream_t)stream, b->ev_side, 0));
  }
  return rc;
}

extern "C" int scalce_batch_finish(scalce_batch *b, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
  HIP_TRY(b->ctx, hipStreamSynchronize(s));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_err(b->ctx, "kernel launch failed: %s", hipGetErrorString(e)); return SCALCE_ERR_HIP; }
  { int rc = entropy_collect(b, s); if (rc) return rc; }
  return check_device_error(b, s);
}

extern "C" uint64_t scalce_batch_reads(const scalce_batch *b) { return b ? b->N : 0; }
extern "C" int scalce_batch_params(const scalce_batch *b, scalce_params *out) {
  if (!b || !out) return SCALCE_ERR_ARG;
  *out = b->p;
  return SCALCE_OK;
}

// the first two and the last two q' symbols of the rows held (input order), and how many symbols there are: what a rank of a
// sharded run tells its neighbours (the trigrams that straddle a rank boundary) -- without asking for SCALCE_OUT_QINPUT as
// one array, which fused rows would have to be copied together for
extern "C" int scalce_batch_qinput_edges(scalce_batch *b, int mate, uint8_t edge[4], uint64_t *nsym, int32_t *read_len, void *stream) {
  if (!b || mate < 0 || mate >= b->nm || !edge || !nsym || b->nq) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  const u64 L = (u64)b->L[mate], n = b->N * L, QS = b->qstride[mate];
  *nsym = n;
  if (read_len) *read_len = b->L[mate];
  edge[0] = edge[1] = edge[2] = edge[3] = 0;
  const u8 *q = b->ws->q[mate].as<u8>();
  auto at = [&](u64 t) { return q + (t / L) * QS + (t % L); };
  // (on the caller's stream, behind the ingest: a device-wide wait would sit behind every coder that is running)
  if (n >= 2) {
    HIP_TRY(c, hipMemcpyAsync(&edge[0], at(0), 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&edge[1], at(1), 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&edge[2], at(n - 2), 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&edge[3], at(n - 1), 1, hipMemcpyDeviceToHost, s));
  } else if (n == 1) {
    HIP_TRY(c, hipMemcpyAsync(&edge[0], at(0), 1, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (n == 1) edge[3] = edge[0];
  return SCALCE_OK;
}

extern "C" int scalce_batch_set_frame_on_demand(scalce_batch *b, int on) {
  if (!b) return SCALCE_ERR_ARG;
  b->frame_on_demand = on != 0;
  return SCALCE_OK;
}

extern "C" int scalce_batch_qual_bytes(const scalce_batch *b, int mate, uint64_t *nbytes) {
  if (!b || !nbytes || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  *nbytes = b->out_qual_bytes[mate];
  return SCALCE_OK;
}

// bytes [offset, offset + nbytes) of mate's framed quality stream -> dst (device memory, or pinned host memory: the
// kernel's stores go over the link), straight from the coder's block buffers when the frames are only laid out
extern "C" int scalce_batch_qual_window(scalce_batch *b, int mate, uint64_t offset, uint64_t nbytes, void *dst, void *stream) {
  if (!b || mate < 0 || mate >= b->nm || (nbytes && !dst)) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  if (b->ent_pending[mate] || b->frame_deferred[mate]) { set_err(c, "collect the entropy stage first (scalce_batch_finish)"); return SCALCE_ERR_ARG; }
  if (offset > b->out_qual_bytes[mate] || nbytes > b->out_qual_bytes[mate] - offset) { set_err(c, "window beyond the stream"); return SCALCE_ERR_ARG; }
  if (!nbytes) return SCALCE_OK;
  if (b->p.no_ac || !b->frame_virtual[mate]) {  // the stream exists as such
    const u8 *src = b->p.no_ac ? b->qs(mate).as<u8>() : b->out_qual[mate].as<u8>();
    HIP_TRY(c, hipMemcpyAsync(dst, src + offset, nbytes, hipMemcpyDefault, s));
    return SCALCE_OK;
  }
  if ((uintptr_t)dst & 3) { set_err(c, "window destination must be 4-byte aligned"); return SCALCE_ERR_ARG; }
  // the blocks whose frames meet the window
  const std::vector<u64> &off = b->frame_off_host[mate];
  const u32 nblk = b->frame_virtual[mate];
  if (off.size() != (size_t)nblk) { set_err(c, "internal: frame layout not collected"); return SCALCE_ERR_ARG; }
  const u32 b0 = (u32)(std::upper_bound(off.begin(), off.end(), (u64)offset) - off.begin()) - 1u;  // off[0] = 0 <= offset
  const u32 b1 = (u32)(std::lower_bound(off.begin(), off.end(), (u64)(offset + nbytes)) - off.begin());
  LAUNCH(ac_frame_window_k, dim3(cdiv(b->ac_stride[mate], 16 * 256), b1 - b0), 256, 0, s, b->ac_base[mate], b->ac_stride[mate],
         b->ac_sizes[mate].as<u32>(), b->ac_off[mate].as<u64>(), (u64)offset, (u64)(offset + nbytes), static_cast<u8 *>(dst), b0);
  return launch_failed(c);
}

// SCALCE_OUT_QUAL as one device buffer for callers that want that: the frames laid out by entropy_collect are copied now
static int materialize_frames(scalce_batch *b, int m) {
  if (!b->frame_virtual[m]) return SCALCE_OK;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  ENSURE(b, b->out_qual[m], (size_t)b->out_qual_bytes[m] + 64);
  LAUNCH(ac_frame_k, dim3(cdiv(b->ac_stride[m], 16 * 256), b->frame_virtual[m]), 256, 0, (hipStream_t) nullptr, b->ac_base[m], b->ac_stride[m],
         b->ac_sizes[m].as<u32>(), b->ac_off[m].as<u64>(), b->out_qual[m].as<u8>());
  HIP_TRY(c, hipDeviceSynchronize());
  b->frame_virtual[m] = 0;
  return launch_failed(c);
}

extern "C" int scalce_batch_output(const scalce_batch *b, int which, int mate, const void **d_ptr, uint64_t *nbytes) {
  if (!b || !d_ptr || !nbytes || mate < 0 || mate >= b->nm) return SCALCE_ERR_ARG;
  const scalce_workspace &w = *b->ws;
  const u32 nb1 = (u32)b->ctx->A.n_buckets + 1;
  if (b->nq && (which == SCALCE_OUT_QUAL || which == SCALCE_OUT_TABLE || which == SCALCE_OUT_FREQ4 || which == SCALCE_OUT_QSTREAM ||
                which == SCALCE_OUT_QINPUT)) {  // -Q / -f: nothing quality-side exists
    *d_ptr = nullptr;
    *nbytes = 0;
    return SCALCE_OK;
  }
  if (which == SCALCE_OUT_QUAL && !b->p.no_ac && b->frame_virtual[mate]) {
    int rc = materialize_frames(const_cast<scalce_batch *>(b), mate);
    if (rc) return rc;
  }
  switch (which) {
    case SCALCE_OUT_READS: *d_ptr = b->out_reads[mate].p; *nbytes = b->out_reads_bytes[mate]; break;
    case SCALCE_OUT_NAMES: *d_ptr = b->out_names.p; *nbytes = b->out_names_bytes; break;
    case SCALCE_OUT_QUAL:
      *d_ptr = b->p.no_ac ? b->qs(mate).p : b->out_qual[mate].p;
      *nbytes = b->out_qual_bytes[mate];
      break;
    case SCALCE_OUT_TABLE: *d_ptr = b->table[mate].p; *nbytes = sizeof(u32) * 512000; break;
    case SCALCE_OUT_FREQ4: *d_ptr = b->freq4[mate].p; *nbytes = sizeof(u64) * 512000; break;
    case SCALCE_OUT_TOKENS: *d_ptr = w.tokens.p; *nbytes = sizeof(int32_t) * 2 * b->N; break;
    case SCALCE_OUT_PERM: *d_ptr = b->perm; *nbytes = sizeof(u32) * b->N; break;
    case SCALCE_OUT_QSTREAM: *d_ptr = b->qs(mate).p; *nbytes = b->N * (u64)b->L[mate]; break;
    case SCALCE_OUT_BUCKET_COUNTS: *d_ptr = b->tok_open ? w.counts.p : b->counts_total.p; *nbytes = sizeof(u64) * nb1; break;
    case SCALCE_OUT_QINPUT:
      *nbytes = b->N * (u64)b->L[mate];
      if (b->qstride[mate] == (u32)b->L[mate]) { *d_ptr = w.q[mate].p; break; }
      {  // fused rows: the q' of every row as one array, put together on request
        scalce_batch *mb = const_cast<scalce_batch *>(b);
        if (hipSetDevice(b->ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SCALCE_ERR_HIP;
        int rc = ensure(mb, mb->q_compact, (size_t)*nbytes + 64);
        if (rc) return rc;
        if (b->N) LAUNCH(compact_q_k, 4096, 256, 0, (hipStream_t) nullptr, b->N, w.q[mate].as<u8>(), b->qstride[mate], (u32)b->L[mate], mb->q_compact.as<u8>());
        if (hipDeviceSynchronize() != hipSuccess) return SCALCE_ERR_HIP;
        *d_ptr = mb->q_compact.p;
      }
      break;
    case SCALCE_OUT_NAMELEN: *d_ptr = w.namelen.p; *nbytes = b->N; break;
    case SCALCE_OUT_LENGTHS: *d_ptr = b->out_lengths[mate].p; *nbytes = b->vl && b->out_lengths[mate].p ? sizeof(u16) * b->N : 0; break;
    case SCALCE_OUT_BUCKET_NAME_BYTES: *d_ptr = b->bucket_name_bytes.p; *nbytes = b->bucket_name_bytes.p ? sizeof(u64) * nb1 : 0; break;
    case SCALCE_OUT_COMMENTS:
      *d_ptr = b->keep_comments ? b->out_comments[mate].p : nullptr;
      *nbytes = b->keep_comments && b->out_comments[mate].p ? b->out_comments_bytes[mate] : 0;
      break;
    case SCALCE_OUT_EXCEPTIONS:
      *d_ptr = b->keep_bases ? b->out_exc[mate].p : nullptr;
      *nbytes = b->keep_bases && b->out_exc[mate].p ? sizeof(u64) * b->out_exc_entries[mate] : 0;
      break;
    case SCALCE_OUT_PLUS:
      *d_ptr = b->keep_plus ? b->out_plus[mate].p : nullptr;
      *nbytes = b->keep_plus && b->out_plus[mate].p ? b->out_plus_bytes[mate] : 0;
      break;
    case SCALCE_OUT_NAMECELLS: *d_ptr = w.namecell.p; *nbytes = b->p.use_names && w.namecell.p ? 16 * b->N : 0; break;
    default: return SCALCE_ERR_ARG;
  }
  return SCALCE_OK;
}

extern "C" int scalce_batch_stage_ms(scalce_batch *b, int which, float *ms, int *launches) {
  if (!b || which < 0 || which >= ST_COUNT) return SCALCE_ERR_ARG;
  if (ms) *ms = b->stage_ms[which];
  if (launches) *launches = b->stage_launches[which];
  return SCALCE_OK;
}
extern "C" void scalce_batch_stage_reset(scalce_batch *b, int enable) {
  if (!b) return;
  b->timing = enable != 0;
  for (int i = 0; i < ST_COUNT; i++) { b->stage_ms[i] = 0; b->stage_launches[i] = 0; }
}

extern "C" void scalce_batch_kernel_timing(scalce_batch *b, int enable) {
  if (!b) return;
  b->ktiming = enable != 0;
  b->kev_used = 0;
  b->k_in_bytes = b->k_out_bytes = 0;
}
extern "C" int scalce_batch_kernel_ms(scalce_batch *b, double *total_ms, int *launches, uint64_t *bytes_in,
                                      uint64_t *bytes_out) {
  if (!b) return SCALCE_ERR_ARG;
  double tot = 0;
  for (size_t i = 0; i < b->kev_used; i++) {
    float ms = 0;
    HIP_TRY(b->ctx, hipEventSynchronize(b->kev[i].second));
    HIP_TRY(b->ctx, hipEventElapsedTime(&ms, b->kev[i].first, b->kev[i].second));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int)b->kev_used;
  if (bytes_in) *bytes_in = b->k_in_bytes;
  if (bytes_out) *bytes_out = b->k_out_bytes;
  return SCALCE_OK;
}

extern "C" int scalce_memcpy_d2h(scalce_ctx *c, void *dst, const void *src, uint64_t n) {
  if (!c) return SCALCE_ERR_ARG;
  if (!n) return SCALCE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  return SCALCE_OK;
}
extern "C" int scalce_memcpy_h2d(scalce_ctx *c, void *dst, const void *src, uint64_t n) {
  if (!c) return SCALCE_ERR_ARG;
  if (!n) return SCALCE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
  return SCALCE_OK;
}
extern "C" int scalce_memcpy_d2d(scalce_ctx *c, void *dst, const void *src, uint64_t n, void *stream) {
  if (!c) return SCALCE_ERR_ARG;
  if (!n) return SCALCE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SCALCE_OK;
}
extern "C" int scalce_batch_stats(const scalce_batch *b, uint32_t out[7]) {
  if (!b || !out) return SCALCE_ERR_ARG;
  out[0] = b->ntie; out[1] = b->nev; out[2] = b->jacobi_iters; out[3] = b->nchunks;
  out[4] = b->order_run_members;
  out[5] = b->tie_fallback ? 1u : 0u;
  out[6] = b->order_radix_fallback;
  return SCALCE_OK;
}
extern "C" int scalce_batch_tie_plan(const scalce_batch *b, uint32_t out[4]) {
  if (!b || !out) return SCALCE_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = b->tie_plan[i];
  return SCALCE_OK;
}

extern "C" int scalce_selftest_ac(scalce_ctx *c, uint64_t ncases, uint32_t seed, int general, uint32_t out[6]) {
  if (!c || !out) return SCALCE_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u32 *d = nullptr;
  HIP_TRY(c, hipMalloc(&d, 8 * sizeof(u32)));
  HIP_TRY(c, hipMemset(d, 0, 8 * sizeof(u32)));
  LAUNCH(ac_selftest_k, cdiv(ncases, 256), 256, 0, 0, (u64)ncases, seed, general, d);
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(out, d, 6 * sizeof(u32), hipMemcpyDeviceToHost));
  hipFree(d);
  return SCALCE_OK;
}
