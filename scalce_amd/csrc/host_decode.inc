// host_decode.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): the inverse path: arithmetic decoder dispatch and records -> FASTQ text
// ---- decode ---------------------------------------------------------------------------------------------
#include <memory>
// What depends only on the table, prepared once per archive: the interval table (ac_table_k), the compact rows
// (ac_dec_rows_k), the ranking of the hot symbols and the choice between ac_decode_tight_k and ac_decode_k.  A launch then
// takes a run of whole frames that starts at any frame of the stream.
struct scalce_ac_decoder {
  scalce_ctx *c = nullptr;
  DBuf d_table, d_cum;  // u32 (d_cum: ac_table_k writes the cumulative counts beside the intervals)
  DBuf d_tab;           // uint4
  DBuf d_rows;          // uint2
  bool cached = false, tight = false;
  int wpb_forced = -1;    // test hook SCALCE_AC_DECODE_WPB: chains per workgroup (2, 4, 8, 16); 0 = the plain decoder
  AcDecCachedArgs ca;
};
extern "C" void scalce_ac_decoder_destroy(scalce_ac_decoder *d) {
  if (!d) return;
  (void)hipSetDevice(d->c->device);
  delete d;
}
extern "C" uint64_t scalce_ac_decoder_device_bytes(const scalce_ac_decoder *d) {
  return d ? d->d_table.cap + d->d_cum.cap + d->d_tab.cap + d->d_rows.cap : 0;
}
extern "C" int scalce_ac_decoder_create(scalce_ctx *c, const uint32_t *table_host, void *stream, scalce_ac_decoder **out) {
  if (!c || !table_host || !out) return SCALCE_ERR_ARG;
  *out = nullptr;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  std::unique_ptr<scalce_ac_decoder, void (*)(scalce_ac_decoder *)> d(new scalce_ac_decoder, scalce_ac_decoder_destroy);
  d->c = c;
  memset(&d->ca, 0, sizeof d->ca);
  HIP_TRY(c, dbuf_alloc(d->d_table, sizeof(u32) * 512000));
  HIP_TRY(c, dbuf_alloc(d->d_tab, sizeof(uint4) * 512000));
  HIP_TRY(c, dbuf_alloc(d->d_cum, sizeof(u32) * 6400 * 81));
  HIP_TRY(c, hipMemcpyAsync(d->d_table.p, table_host, sizeof(u32) * 512000, hipMemcpyHostToDevice, s));
  LAUNCH(ac_table_k, cdiv(6400, 64), 64, 0, s, d->d_table.as<u32>(), d->d_tab.as<uint4>(), d->d_cum.as<u32>(), (u32 *)nullptr);
  // span of the symbols that occur (scaled count > 1 in some context) and their totals: what the compact rows hold and
  // which contexts go to LDS.  (A symbol outside the span can still be coded -- one occurrence scales down to the
  // floor count 1 -- and takes the full-row path in the kernel.)
  u32 smin = AC_D, smax = 0;
  std::vector<u64> tot(AC_D, 0);
  for (u32 ctx = 0; ctx < 6400; ctx++)
    for (u32 sy = 0; sy < AC_D; sy++) {
      const u32 v = table_host[(size_t)ctx * AC_D + sy];
      if (v > 1) { smin = std::min(smin, sy); smax = std::max(smax, sy); tot[sy] += v; }
    }
  const char *wpb_env = getenv("SCALCE_AC_DECODE_WPB");
  if (wpb_env) d->wpb_forced = atoi(wpb_env);
  d->cached = smin <= smax && smax - smin + 2 <= 64 && d->wpb_forced != 0;
  if (d->cached) {
    AcDecCachedArgs &ca = d->ca;
    ca.smin = smin;
    ca.S1 = smax - smin + 2;
    std::vector<u32> order;
    for (u32 sy = smin; sy <= smax; sy++) if (tot[sy]) order.push_back(sy);
    std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return tot[x] > tot[y]; });
    u32 W = 1;
    while (W < 32 && W < order.size() && (u64)(W + 1) * (W + 1) * ca.S1 <= AC_DEC_CACHE_ENTRIES) W++;
    ca.W = W;
    memset(ca.rank, 0xFF, sizeof ca.rank);
    for (u32 r = 0; r < W; r++) { ca.hot[r] = (u8)order[r]; ca.rank[order[r]] = (u8)r; }
    HIP_TRY(c, dbuf_alloc(d->d_rows, sizeof(uint2) * (6400 * ca.S1 + 64)));  // (+ 64: a row is read with all lanes)
    HIP_TRY(c, hipMemsetAsync(d->d_rows.as<uint2>() + 6400 * (size_t)ca.S1, 0, sizeof(uint2) * 64, s));
    LAUNCH(ac_dec_rows_k, cdiv(6400u * ca.S1, 256), 256, 0, s, d->d_tab.as<uint4>(), smin, ca.S1, d->d_rows.as<uint2>());
    ca.rows = d->d_rows.as<uint2>();
    // ONE cached decoder (round 5; rounds 2-4 kept four): ac_decode_tight_k, the loop written by hand for the scalar unit.  It
    // needs what every table of quality strings gives -- no symbol 79 among those that occur (that symbol marks "last of its
    // context" in the rows) and no context total above 2^29 (as for the encoder's plain step); any other table takes the plain
    // decoder, the reference's own loop (arithmetic.cpp:196-268) a wavefront per block.
    u64 max_total = 0;
    for (u32 ctx = 0; ctx < 6400; ctx++) {
      u64 t = 0;
      for (u32 sy = 0; sy < AC_D; sy++) t += table_host[(size_t)ctx * AC_D + sy];
      max_total = std::max(max_total, t);
    }
    d->tight = smax < AC_D - 1 && max_total <= (1ull << 29);
  }
  HIP_TRY(c, hipStreamSynchronize(s));  // (table_host is the caller's again)
  if (int rc = launch_failed(c)) return rc;
  *out = d.release();
  return SCALCE_OK;
}
// Enqueues the decode of `nframes` whole frames that begin at d_frames (nbytes of them are there) into d_out: nsym symbols,
// AC_BLOCK_SYMS per frame but the last.  d_off / d_size (nframes entries) and d_bad (one word) are the caller's scratch: the
// walk fills them and the decoder reads them, nothing comes back to the host in between -- the caller reads *d_bad once the
// stream has got there.  Nothing is allocated and nothing waits.
extern "C" int scalce_ac_decoder_launch(scalce_ac_decoder *d, const uint8_t *d_frames, uint64_t nbytes, uint32_t nframes,
                                        uint64_t nsym, uint64_t *d_off, uint32_t *d_size, uint32_t *d_bad, uint8_t *d_out,
                                        void *stream) {
  if (!d || !d_frames || !d_off || !d_size || !d_bad || !d_out) return SCALCE_ERR_ARG;
  if (!nframes) return SCALCE_OK;
  if (nsym > (u64)nframes * AC_BLOCK_SYMS || nsym <= (u64)(nframes - 1) * AC_BLOCK_SYMS) return SCALCE_ERR_ARG;
  scalce_ctx *c = d->c;
  hipStream_t s = (hipStream_t)stream;
  const u32 nblk = nframes;
  // the walk is serial by nature (each size says where the next one is): a small kernel follows the chain of this launch's frames
  LAUNCH(ac_frame_walk_k, 1, 1, 0, s, d_frames, (u64)nbytes, nblk, reinterpret_cast<u64 *>(d_off), d_size, d_bad);
  AcDecArgs a;
  a.in = d_frames; a.blk_off = reinterpret_cast<const u64 *>(d_off); a.blk_size = d_size; a.nsym = nsym; a.tab = d->d_tab.as<uint4>(); a.out = d_out;
  if (d->cached && d->tight) {
    AcDecCachedArgs ca = d->ca;
    ca.d = a;
    ca.nblk = nblk;
    // Waves of a workgroup share the LDS cache of hot rows (one workgroup per CU): two chains per workgroup keep the
    // latency of a block lowest; from 512 blocks on, eight per workgroup -- two chains per SIMD interleave their issue
    // slots -- put four times as many blocks in flight.  The choice follows the frames of THIS launch.
    int wpb = nblk <= 512 ? 2 : nblk <= 1024 ? 4 : nblk <= 2048 ? 8 : 16;  // 16 = four chains per SIMD: a chain issues one instruction in five cycles
    if (d->wpb_forced > 0) wpb = d->wpb_forced;
    if (wpb == 2) LAUNCH(ac_decode_tight_k<2>, cdiv(nblk, 2), 128, 0, s, ca);
    else if (wpb == 4) LAUNCH(ac_decode_tight_k<4>, cdiv(nblk, 4), 256, 0, s, ca);
    else if (wpb == 16) LAUNCH(ac_decode_tight_k<16>, cdiv(nblk, 16), 1024, 0, s, ca);
    else LAUNCH(ac_decode_tight_k<8>, cdiv(nblk, 8), 512, 0, s, ca);
  } else {
    LAUNCH(ac_decode_k, nblk, 64, 0, s, a);
  }
  return launch_failed(c);
}

// the whole stream at once: a decoder made for this call, one launch over all its frames
extern "C" int scalce_ac_decode(scalce_ctx *c, const uint32_t *table_host, const uint8_t *d_blocks, uint64_t nbytes,
                                uint64_t nsym, uint8_t *d_out, void *stream) {
  if (!c || !table_host || !d_blocks || !d_out) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  const u32 nblk = cdiv(nsym, AC_BLOCK_SYMS);
  if (!nblk) return SCALCE_OK;
  scalce_ac_decoder *made = nullptr;
  if (int rc = scalce_ac_decoder_create(c, table_host, stream, &made)) return rc;
  std::unique_ptr<scalce_ac_decoder, void (*)(scalce_ac_decoder *)> dec(made, scalce_ac_decoder_destroy);
  DBuf d_off, d_sz;  // u64 offsets; u32: nblk sizes and, behind them, the walk's verdict
  u32 bad = 0;
  auto hip_failed = [&](hipError_t e) {
    if (e != hipSuccess) set_err(c, "decoding the quality stream: %s", hipGetErrorString(e));
    return e != hipSuccess;
  };
  if (hip_failed(dbuf_alloc(d_off, sizeof(u64) * nblk)) || hip_failed(dbuf_alloc(d_sz, sizeof(u32) * ((size_t)nblk + 1)))) return SCALCE_ERR_HIP;
  u32 *sz = d_sz.as<u32>();
  if (int rc = scalce_ac_decoder_launch(dec.get(), d_blocks, nbytes, nblk, nsym, d_off.as<uint64_t>(), sz, sz + nblk, d_out, stream)) return rc;
  if (hip_failed(hipMemcpyAsync(&bad, sz + nblk, sizeof bad, hipMemcpyDeviceToHost, s)) || hip_failed(hipStreamSynchronize(s))) return SCALCE_ERR_HIP;
  if (bad) { set_err(c, "(ERROR) truncated quality stream"); return SCALCE_ERR_FORMAT; }
  return SCALCE_OK;
}

// ---- decode side, records -> FASTQ text (SURVEY 8f-1; decompress.cpp:240-366) -----------------------------------
extern "C" uint64_t scalce_fastq_text_bytes(int read_len, uint64_t nrecords, uint64_t names_bytes, const char *library) {
  const u64 L = (u64)read_len, N = nrecords;
  if (!library) return names_bytes - N + N * (2 * L + 6);  // names_bytes = sum of (1 + n)
  u64 digits = N, p = 10;  // digits of 0 .. N-1
  for (int t = 2; t <= 20 && N > p; t++, p *= 10) digits += N - p;
  return N * (strlen(library) + 2 * L + 7) + digits;
}
extern "C" uint64_t scalce_fasta_text_bytes(int read_len, uint64_t nrecords, uint64_t names_bytes, const char *library) {
  const u64 L = (u64)read_len, N = nrecords;
  if (!library) return names_bytes - N + N * (L + 3);  // "@" name "\n" bases "\n"
  u64 digits = N, p = 10;
  for (int t = 2; t <= 20 && N > p; t++, p *= 10) digits += N - p;
  return N * (strlen(library) + L + 4) + digits;
}

// where every name starts (each length byte says where the next one is: serial); false: the stream is short
static bool name_offsets(const uint8_t *names_host, uint64_t names_bytes, uint64_t nrecords, std::vector<u64> &name_off) {
  name_off.resize(nrecords + 1);
  u64 pos = 0;
  for (u64 k = 0; k < nrecords; k++) {
    if (pos >= names_bytes) return false;
    name_off[k] = pos;
    pos += 1 + (u64)names_host[pos];
  }
  if (pos > names_bytes) return false;
  name_off[nrecords] = pos;
  return true;
}
// a wavefront per FQ_RECORDS_PER_WAVE records of the window (or archive) that `a` describes
static void launch_records(const FqArgs &a, bool qual, hipStream_t s) {
  const u64 waves = (a.nrecords + FQ_RECORDS_PER_WAVE - 1) / FQ_RECORDS_PER_WAVE;
  if (qual) LAUNCH(fastq_records_k<true>, cdiv(waves, 4), 256, 0, s, a);
  else LAUNCH(fastq_records_k<false>, cdiv(waves, 4), 256, 0, s, a);
}
static_assert(sizeof(scalce_fq_bucket) == sizeof(FqBucket) && offsetof(scalce_fq_bucket, core) == offsetof(FqBucket, core) &&
              offsetof(scalce_fq_bucket, rec_bytes) == offsetof(FqBucket, rec_bytes), "scalce_fq_bucket is FqBucket");
// One window of whole records, everything resident and window-relative (scalce_fq_window): enqueues the kernel, nothing else
extern "C" int scalce_fastq_records_window(scalce_ctx *c, const scalce_fq_window *w, void *stream) {
  if (!c || !w || w->read_len <= 0 || !w->d_reads || !w->d_dir || !w->nbuckets || !w->d_out) return SCALCE_ERR_ARG;
  if ((w->d_names != nullptr) != (w->d_name_off != nullptr) || (!w->d_names && !w->library)) return SCALCE_ERR_ARG;
  if (w->interleave && w->d_names && !w->d_pair_name_off) return SCALCE_ERR_ARG;
  if (!w->nrecords) return SCALCE_OK;
  FqArgs a;
  memset(&a, 0, sizeof a);
  if (!w->d_names) {
    const size_t n = strlen(w->library);
    if (n >= sizeof a.lib) { set_err(c, "library name longer than %zu characters", sizeof a.lib - 1); return SCALCE_ERR_ARG; }
    a.lib_len = (u32)n;
    memcpy(a.lib, w->library, n);
  }
  a.reads = w->d_reads; a.dir = reinterpret_cast<const FqBucket *>(w->d_dir); a.nbuckets = w->nbuckets;
  a.nrecords = w->nrecords; a.first = w->first_record; a.L = (u32)w->read_len;
  a.sz_meta = w->has_buckets ? (w->read_len > 255 ? 2u : 1u) : 0u;
  a.qual = w->d_qual; a.phred = (u32)w->phred_offset; a.names = w->d_names; a.name_off = reinterpret_cast<const u64 *>(w->d_name_off);
  a.mate_digit = (u32)w->mate_digit; a.out = w->d_out; a.rec_off = reinterpret_cast<u64 *>(w->d_record_offsets);
  a.il = (u32)w->interleave; a.pair_L = (u32)w->pair_read_len; a.pair_name_off = reinterpret_cast<const u64 *>(w->d_pair_name_off);
  launch_records(a, w->d_qual != nullptr, (hipStream_t)stream);
  return launch_failed(c);
}

// -d -i: this mate's records go into the text both mates share (FqArgs::il)
struct FqPairHost {
  u32 il;                        // 1: mate 1, 2: mate 2
  int pair_L;                    // the other mate's read length
  const std::vector<u64> *pair_noff;  // the other mate's name offsets (names mode)
  u64 total;                     // bytes of the whole interleaved text
};
static int fastq_records_impl(scalce_ctx *c, int read_len, int has_buckets, const uint8_t *reads_host, uint64_t reads_bytes,
                              uint64_t nrecords, const uint8_t *d_qual, int64_t phred_offset, const uint8_t *names_host,
                              uint64_t names_bytes, const char *library, int mate_digit, uint8_t *d_out, uint64_t out_cap,
                              uint64_t *out_bytes, uint64_t *record_offsets_host, void *stream, const FqPairHost *pair) {
  if (!c || read_len <= 0 || !reads_host || (!names_host && !library) || !d_out) return SCALCE_ERR_ARG;
  const bool qual = d_qual != nullptr;  // NULL: two-line records of an archive without qualities
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  const u32 L = (u32)read_len;
  const u32 sz_meta = has_buckets ? (L > 255 ? 2u : 1u) : 0u;
  // 1. the bucket directory (decompress.cpp:262-270): headers sit between the buckets' records, so the walk is serial
  std::vector<FqBucket> dir;
  if (has_buckets) {
    u64 pos = 0, k = 0;
    while (pos + 12 <= reads_bytes) {
      int32_t core;
      u64 cnt;
      memcpy(&core, reads_host + pos, 4);
      memcpy(&cnt, reads_host + pos + 4, 8);
      pos += 12;
      FqBucket b;
      memset(&b, 0, sizeof b);
      if (core != SCALCE_ROOT_CORE) {
        if (core < 0 || core >= (int)c->A.patterns.size()) {
          set_err(c, "(ERROR) archive refers to core %d which the core table does not have", core);
          return SCALCE_ERR_FORMAT;
        }
        const std::string &cs = c->A.patterns[core];
        if (cs.size() > sizeof b.core || cs.size() > L) { set_err(c, "(ERROR) core %d does not fit the reads", core); return SCALCE_ERR_FORMAT; }
        b.core_len = (u32)cs.size();
        memcpy(b.core, cs.data(), cs.size());
      }
      b.first = k;
      b.off = pos;
      b.rec_bytes = (L - b.core_len + 3) / 4 + sz_meta;
      if (cnt > (reads_bytes - pos) / b.rec_bytes) { set_err(c, "(ERROR) truncated read stream"); return SCALCE_ERR_FORMAT; }
      pos += cnt * b.rec_bytes;
      k += cnt;
      if (cnt) dir.push_back(b);
    }
    if (k != nrecords) {
      set_err(c, "(ERROR) the read stream holds %llu records, the quality stream %llu", (unsigned long long)k, (unsigned long long)nrecords);
      return SCALCE_ERR_FORMAT;
    }
  } else {
    FqBucket b;
    memset(&b, 0, sizeof b);
    b.rec_bytes = (L + 3) / 4;
    if (nrecords > reads_bytes / b.rec_bytes) { set_err(c, "(ERROR) truncated read stream"); return SCALCE_ERR_FORMAT; }
    dir.push_back(b);
  }
  // 2. where every name starts (each length byte says where the next one is: serial as well)
  std::vector<u64> name_off;
  if (names_host) {
    if (!name_offsets(names_host, names_bytes, nrecords, name_off)) { set_err(c, "(ERROR) truncated name stream"); return SCALCE_ERR_FORMAT; }
    names_bytes = name_off[nrecords];
  }
  const u64 total = pair ? pair->total
                         : (qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes)(read_len, nrecords, names_bytes, names_host ? nullptr : library);
  if (out_bytes) *out_bytes = total;
  if (total > out_cap) { set_err(c, "output buffer of %llu bytes, the text needs %llu", (unsigned long long)out_cap, (unsigned long long)total); return SCALCE_ERR_CAPACITY; }
  if (!nrecords) return SCALCE_OK;
  FqArgs a;
  memset(&a, 0, sizeof a);
  DBuf d_reads, d_names, d_dir, d_noff, d_roff, d_pnoff;  // (gone with the call, on every way out)
#define FQ_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { set_err(c, "%s failed: %s", #expr, hipGetErrorString(e_)); return SCALCE_ERR_HIP; } } while (0)
  FQ_TRY(dbuf_alloc(d_reads, reads_bytes + 64));
  FQ_TRY(dbuf_alloc(d_dir, sizeof(FqBucket) * dir.size()));
  FQ_TRY(hipMemcpyAsync(d_reads.p, reads_host, reads_bytes, hipMemcpyHostToDevice, s));
  FQ_TRY(hipMemcpyAsync(d_dir.p, dir.data(), sizeof(FqBucket) * dir.size(), hipMemcpyHostToDevice, s));
  if (names_host) {
    FQ_TRY(dbuf_alloc(d_names, names_bytes + 64));
    FQ_TRY(dbuf_alloc(d_noff, sizeof(u64) * (nrecords + 1)));
    FQ_TRY(hipMemcpyAsync(d_names.p, names_host, names_bytes, hipMemcpyHostToDevice, s));
    FQ_TRY(hipMemcpyAsync(d_noff.p, name_off.data(), sizeof(u64) * (nrecords + 1), hipMemcpyHostToDevice, s));
    if (pair) {
      FQ_TRY(dbuf_alloc(d_pnoff, sizeof(u64) * (nrecords + 1)));
      FQ_TRY(hipMemcpyAsync(d_pnoff.p, pair->pair_noff->data(), sizeof(u64) * (nrecords + 1), hipMemcpyHostToDevice, s));
    }
  } else {
    a.lib_len = (u32)std::min<size_t>(strlen(library), sizeof a.lib - 1);
    if (strlen(library) >= sizeof a.lib) { set_err(c, "library name longer than %zu characters", sizeof a.lib - 1); return SCALCE_ERR_ARG; }
    memcpy(a.lib, library, a.lib_len);
  }
  if (record_offsets_host) FQ_TRY(dbuf_alloc(d_roff, sizeof(u64) * (nrecords + 1)));
  a.reads = d_reads.as<u8>(); a.dir = d_dir.as<FqBucket>(); a.nbuckets = (u32)dir.size(); a.nrecords = nrecords; a.L = L; a.sz_meta = sz_meta;
  a.qual = d_qual; a.phred = (u32)phred_offset; a.names = d_names.as<u8>(); a.name_off = d_noff.as<u64>();
  a.mate_digit = (u32)mate_digit; a.out = d_out; a.rec_off = d_roff.as<u64>();
  if (pair) { a.il = pair->il; a.pair_L = (u32)pair->pair_L; a.pair_name_off = d_pnoff.as<u64>(); }
  launch_records(a, qual, s);
  if (record_offsets_host)
    FQ_TRY(hipMemcpyAsync(record_offsets_host, d_roff.p, sizeof(u64) * (nrecords + 1), hipMemcpyDeviceToHost, s));
  FQ_TRY(hipStreamSynchronize(s));
  FQ_TRY(hipGetLastError());
#undef FQ_TRY
  return SCALCE_OK;
}

extern "C" int scalce_fastq_records(scalce_ctx *c, int read_len, int has_buckets, const uint8_t *reads_host, uint64_t reads_bytes,
                                    uint64_t nrecords, const uint8_t *d_qual, int64_t phred_offset, const uint8_t *names_host,
                                    uint64_t names_bytes, const char *library, int mate_digit, uint8_t *d_out, uint64_t out_cap,
                                    uint64_t *out_bytes, uint64_t *record_offsets_host, void *stream) {
  return fastq_records_impl(c, read_len, has_buckets, reads_host, reads_bytes, nrecords, d_qual, phred_offset, names_host, names_bytes,
                            library, mate_digit, d_out, out_cap, out_bytes, record_offsets_host, stream, nullptr);
}

// -d -i: both mates into one text, each by the kernel that writes its own text, at the places the pairs give
extern "C" int scalce_fastq_records_interleaved(scalce_ctx *c, const int read_len[2], const uint8_t *const reads_host[2],
                                                const uint64_t reads_bytes[2], uint64_t npairs, const uint8_t *const d_qual[2],
                                                const int64_t phred_offset[2], const uint8_t *const names_host[2],
                                                const uint64_t names_bytes[2], const char *library, uint8_t *d_out, uint64_t out_cap,
                                                uint64_t *out_bytes, uint64_t *pair_offsets_host, void *stream) {
  if (!c || !read_len || !reads_host || !reads_bytes || !d_qual || !phred_offset || !names_host || !names_bytes || !d_out) return SCALCE_ERR_ARG;
  const bool names = names_host[0] != nullptr;
  if ((names_host[1] != nullptr) != names || (!names && !library) || (d_qual[0] != nullptr) != (d_qual[1] != nullptr)) return SCALCE_ERR_ARG;
  const bool qual = d_qual[0] != nullptr;
  std::vector<u64> noff[2];
  u64 total = 0;
  for (int m = 0; m < 2; m++) {
    u64 nb = names_bytes[m];
    if (names) {
      if (!name_offsets(names_host[m], names_bytes[m], npairs, noff[m])) { set_err(c, "(ERROR) truncated name stream"); return SCALCE_ERR_FORMAT; }
      nb = noff[m][npairs];
    }
    total += (qual ? scalce_fastq_text_bytes : scalce_fasta_text_bytes)(read_len[m], npairs, nb, names ? nullptr : library);
  }
  if (out_bytes) *out_bytes = total;
  if (total > out_cap) { set_err(c, "output buffer of %llu bytes, the text needs %llu", (unsigned long long)out_cap, (unsigned long long)total); return SCALCE_ERR_CAPACITY; }
  for (int m = 0; m < 2; m++) {
    const FqPairHost pr{(u32)(m + 1), read_len[1 - m], &noff[1 - m], total};
    int rc = fastq_records_impl(c, read_len[m], m == 0, reads_host[m], reads_bytes[m], npairs, d_qual[m], phred_offset[m], names_host[m],
                                names_bytes[m], library, '1' + m, d_out, out_cap, nullptr, m == 0 ? pair_offsets_host : nullptr, stream, &pr);
    if (rc) return rc;
  }
  return SCALCE_OK;
}

// ---- variable-length archives: the pad out of a window's text ------------------------------------------------------------
// One scan of the stripped record sizes (it leaves the new record offsets, and the text's size behind them), one copy pass.
extern "C" uint64_t scalce_fastq_strip_ws_bytes(uint64_t nrecords) { return sizeof(u64) * (scan_ws_elems(nrecords) + 64); }
extern "C" int scalce_fastq_strip_window(scalce_ctx *c, int read_len, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets,
                                         const uint8_t *d_entries, int entry_width, uint8_t *d_out, uint64_t *d_out_offsets, void *d_scan_ws,
                                         void *stream) {
  if (!c || read_len <= 0 || read_len > 65535 || (entry_width != 1 && entry_width != 2) || !d_out_offsets || !d_scan_ws) return SCALCE_ERR_ARG;
  if (nrecords && (!d_text || !d_record_offsets || !d_entries || !d_out)) return SCALCE_ERR_ARG;
  if (((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15)) { set_err(c, "strip: the window's texts must be 16-byte aligned"); return SCALCE_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  StripArgs a;
  a.text = d_text; a.rec_off = reinterpret_cast<const u64 *>(d_record_offsets); a.entries = d_entries;
  a.width = (u32)entry_width; a.L = (u32)read_len; a.nrec = nrecords;
  a.dst_off = reinterpret_cast<u64 *>(d_out_offsets); a.dst = d_out;
  exclusive_scan<u64>(StrippedSize{a}, nrecords, StoreTo<u64>{a.dst_off}, static_cast<u64 *>(d_scan_ws), a.dst_off + nrecords, s);
  if (nrecords) {
    // (the grid covers an upper bound of the text known without a read-back -- a record is '@', a name of up to 255 bytes, two
    // lines of L and "+" with four newlines -- and the workgroups behind the text's end return at once)
    const u64 bound = nrecords * (2ull * (u64)read_len + 6 + 256);
    LAUNCH(strip_copy_k, cdiv(bound, VL_SPAN), 256, 0, s, a);
  }
  return launch_failed(c);
}

// ---- what follows the names, back in a window's text (archives made with --keep-comments; kernels_comments.hpp) -------------
// scratch of scalce_fastq_comment_window, in 64-bit words: the newline counts of the entries' tiles, the tiles of the two scans,
// the count itself, the newline index (one entry per record)
static u64 comment_ws_tiles(u64 entry_bytes) { return (entry_bytes + IDX_TILE - 1) / IDX_TILE + 8; }
static u64 comment_ws_scan(u64 nrecords, u64 entry_bytes) { return scan_ws_elems(std::max<u64>(nrecords, comment_ws_tiles(entry_bytes))) + 64; }
extern "C" uint64_t scalce_fastq_comment_ws_bytes(uint64_t nrecords, uint64_t entry_bytes) {
  return sizeof(u64) * (comment_ws_tiles(entry_bytes) + comment_ws_scan(nrecords, entry_bytes) + 8 + nrecords + 8);
}
// the insert pass over nrecords records of `d_text` that begin at d_record_offsets: a record's tail is tail[r & par]
static int comment_window(scalce_ctx *c, const u64 tail[2], u32 par, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets,
                          const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out, uint64_t *d_out_offsets, uint32_t *d_bad, void *d_ws,
                          u64 text_bound, hipStream_t s) {
  u64 *tile = static_cast<u64 *>(d_ws), *scan = tile + comment_ws_tiles(entry_bytes), *nlines = scan + comment_ws_scan(nrecords, entry_bytes);
  u64 *ent_end = nlines + 8;
  // the newline index of the entries: entry r ends at its r-th newline (an index that stays short leaves empty entries, and *d_bad)
  HIP_TRY(c, hipMemsetAsync(nlines, 0, sizeof(u64) * (8 + nrecords), s));
  const u32 ntiles = cdiv(entry_bytes, IDX_TILE);
  if (ntiles) {
    LAUNCH(index_count_k, ntiles, IDX_THREADS, 0, s, d_entries, entry_bytes, tile);
    exclusive_scan<u64>(LoadAs<u64, u64>{tile}, ntiles, StoreTo<u64>{tile}, scan, nlines, s);
    LAUNCH(index_write_k, ntiles, IDX_THREADS, 0, s, d_entries, entry_bytes, tile, ent_end, nrecords);
  }
  LAUNCH(insert_check_k, 1, 1, 0, s, nlines, d_entries, entry_bytes, nrecords, d_bad);
  InsertArgs a;
  a.text = d_text; a.rec_off = reinterpret_cast<const u64 *>(d_record_offsets); a.entries = d_entries; a.entry_bytes = entry_bytes;
  a.ent_end = ent_end; a.tail[0] = tail[0]; a.tail[1] = tail[1]; a.par = par; a.nrec = nrecords;
  a.dst_off = reinterpret_cast<u64 *>(d_out_offsets); a.dst = d_out;
  exclusive_scan<u64>(InsertedSize{a}, nrecords, StoreTo<u64>{a.dst_off}, scan, a.dst_off + nrecords, s);
  // (the grid covers an upper bound of the text known without a read-back; the workgroups behind the text's end return at once)
  if (nrecords) LAUNCH(insert_copy_k, cdiv(text_bound + entry_bytes, VL_SPAN), 256, 0, s, a);
  return launch_failed(c);
}
static u64 comment_tail(int read_len, int has_qualities) { return has_qualities ? 2ull * (u64)read_len + 5 : (u64)read_len + 2; }
extern "C" int scalce_fastq_comment_window(scalce_ctx *c, int read_len, int has_qualities, uint64_t nrecords, const uint8_t *d_text,
                                           const uint64_t *d_record_offsets, const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out,
                                           uint64_t *d_out_offsets, uint32_t *d_bad, void *d_ws, void *stream) {
  if (!c || read_len <= 0 || read_len > 65535 || !d_out_offsets || !d_bad || !d_ws || nrecords > 0xFFFFFFFFull) return SCALCE_ERR_ARG;
  if (nrecords && (!d_text || !d_record_offsets || !d_out)) return SCALCE_ERR_ARG;
  if (entry_bytes && !d_entries) return SCALCE_ERR_ARG;
  if (((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_entries & 15)) {
    set_err(c, "comments: the window's texts and its entries must be 16-byte aligned");
    return SCALCE_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  // (the records' own bound of the text -- scalce_fastq_strip_window's -- a record is '@', a name of up to 255 bytes, the lines and their newlines)
  const u64 tail[2] = {comment_tail(read_len, has_qualities), 0};
  return comment_window(c, tail, 0, nrecords, d_text, d_record_offsets, d_entries, entry_bytes, d_out, d_out_offsets, d_bad, d_ws,
                        nrecords * (2ull * (u64)read_len + 6 + 256), s);
}

// The same for an interleaved window (scalce_fastq_records_window with interleave): 2 npairs records, mate 1's the even ones, and
// their entries in that order.  The records' own offsets are made from the pairs' and mate 2's name offsets, and the pairs' new
// offsets taken from the records' new ones.
static u64 comment_pairs_words(u64 npairs) { return 2 * npairs + 8; }
extern "C" uint64_t scalce_fastq_comment_pairs_ws_bytes(uint64_t npairs, uint64_t entry_bytes) {
  return scalce_fastq_comment_ws_bytes(2 * npairs, entry_bytes) + sizeof(u64) * 2 * comment_pairs_words(npairs);
}
extern "C" int scalce_fastq_comment_window_pairs(scalce_ctx *c, const int read_len[2], int has_qualities, uint64_t npairs, const uint8_t *d_text,
                                                 const uint64_t *d_pair_offsets, const uint64_t *d_name_off2, const uint8_t *d_entries,
                                                 uint64_t entry_bytes, uint8_t *d_out, uint64_t *d_out_pair_offsets, uint32_t *d_bad, void *d_ws,
                                                 void *stream) {
  if (!c || !read_len || !d_out_pair_offsets || !d_bad || !d_ws || npairs > 0x7FFFFFFFull) return SCALCE_ERR_ARG;
  for (int m = 0; m < 2; m++) if (read_len[m] <= 0 || read_len[m] > 65535) return SCALCE_ERR_ARG;
  if (npairs && (!d_text || !d_pair_offsets || !d_name_off2 || !d_out)) return SCALCE_ERR_ARG;
  if (entry_bytes && !d_entries) return SCALCE_ERR_ARG;
  if (((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_entries & 15)) {
    set_err(c, "comments: the window's texts and its entries must be 16-byte aligned");
    return SCALCE_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  const u64 tail[2] = {comment_tail(read_len[0], has_qualities), comment_tail(read_len[1], has_qualities)};
  u64 *rec_off = reinterpret_cast<u64 *>(static_cast<u8 *>(d_ws) + scalce_fastq_comment_ws_bytes(2 * npairs, entry_bytes));
  u64 *new_off = rec_off + comment_pairs_words(npairs);
  LAUNCH(pair_split_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, reinterpret_cast<const u64 *>(d_pair_offsets), reinterpret_cast<const u64 *>(d_name_off2),
         tail[1], rec_off);
  const int rc = comment_window(c, tail, 1, 2 * npairs, d_text, reinterpret_cast<const uint64_t *>(rec_off), d_entries, entry_bytes, d_out,
                                reinterpret_cast<uint64_t *>(new_off), d_bad, d_ws,
                                npairs * (2ull * ((u64)read_len[0] + (u64)read_len[1]) + 12 + 512), s);
  if (rc) return rc;
  LAUNCH(pair_offsets_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, new_off, reinterpret_cast<u64 *>(d_out_pair_offsets));
  return launch_failed(c);
}

// ---- the letters and qualities the archive does not keep, back in a window's text (archives made with --keep-bases) ---------
static int exception_apply(scalce_ctx *c, u8 *d_text, const u64 *rec_off, u32 stride, u32 which, u64 first, u64 nunits, int read_len,
                           int has_qualities, const uint64_t *d_entries, uint64_t nentries, uint32_t *d_bad, hipStream_t s) {
  if (!nentries) return SCALCE_OK;
  ExcApplyArgs a;
  a.text = d_text; a.rec_off = rec_off; a.stride = stride; a.which = which; a.first = first; a.nunits = nunits;
  a.entries = reinterpret_cast<const u64 *>(d_entries); a.nent = nentries;
  a.L = (u32)read_len; a.has_q = has_qualities ? 1u : 0u; a.bad = d_bad;
  LAUNCH(exc_apply_k, cdiv(nentries, 256), 256, 0, s, a);
  return SCALCE_OK;
}
static bool exception_args_ok(int read_len, uint64_t n, uint64_t nentries, const void *d_text, const void *d_off, const void *d_entries) {
  return read_len > 0 && read_len < (1 << EXC_POS_BITS) && n <= 0xFFFFFFFFull && (!nentries || (d_text && d_off && d_entries && n));
}
extern "C" int scalce_fastq_exception_window(scalce_ctx *c, int read_len, int has_qualities, uint64_t first_record, uint64_t nrecords,
                                             uint8_t *d_text, const uint64_t *d_record_offsets, const uint64_t *d_entries, uint64_t nentries,
                                             uint32_t *d_bad, void *stream) {
  if (!c || !d_bad || !exception_args_ok(read_len, nrecords, nentries, d_text, d_record_offsets, d_entries)) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(u32), s));
  { int rc = exception_apply(c, d_text, reinterpret_cast<const u64 *>(d_record_offsets), 1, 0, first_record, nrecords, read_len, has_qualities,
                             d_entries, nentries, d_bad, s); if (rc) return rc; }
  return launch_failed(c);
}
// The same for an interleaved window: npairs pairs, mate 1 then mate 2 of each; mate m's entries count pairs.  The records'
// own offsets are made from the pairs' and mate 2's name offsets (pair_split_k), then each mate's entries go to its records.
extern "C" uint64_t scalce_fastq_exception_pairs_ws_bytes(uint64_t npairs) { return sizeof(u64) * (2 * npairs + 8); }
extern "C" int scalce_fastq_exception_window_pairs(scalce_ctx *c, const int read_len[2], int has_qualities, uint64_t first_pair, uint64_t npairs,
                                                   uint8_t *d_text, const uint64_t *d_pair_offsets, const uint64_t *d_name_off2, uint64_t library_len,
                                                   const uint64_t *const d_entries[2], const uint64_t nentries[2], uint32_t *d_bad, void *d_ws,
                                                   void *stream) {
  if (!c || !d_bad || !read_len || !d_entries || !nentries || !d_ws || npairs > 0x7FFFFFFFull) return SCALCE_ERR_ARG;
  for (int m = 0; m < 2; m++)
    if (!exception_args_ok(read_len[m], npairs, nentries[m], d_text, d_pair_offsets, d_entries[m])) return SCALCE_ERR_ARG;
  if (!d_name_off2 && library_len > 255) { set_err(c, "exceptions: a library name is at most 255 characters long"); return SCALCE_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(u32), s));
  if (!npairs) return SCALCE_OK;
  u64 *rec_off = static_cast<u64 *>(d_ws);
  if (d_name_off2)
    LAUNCH(pair_split_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, reinterpret_cast<const u64 *>(d_pair_offsets), reinterpret_cast<const u64 *>(d_name_off2),
           comment_tail(read_len[1], has_qualities), rec_off);
  else  // made-up names: "<library>.<index>"
    LAUNCH(pair_split_lib_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, reinterpret_cast<const u64 *>(d_pair_offsets), first_pair, (u32)library_len,
           comment_tail(read_len[1], has_qualities), rec_off);
  for (u32 m = 0; m < 2; m++) {
    int rc = exception_apply(c, d_text, rec_off, 2, m, first_pair, npairs, read_len[m], has_qualities, d_entries[m], nentries[m], d_bad, s);
    if (rc) return rc;
  }
  return launch_failed(c);
}

// ---- the '+' lines, back in a window's text (archives made with --keep-plus; kernels_plus.hpp) --------------------------------
// scratch of scalce_fastq_plus_window, in 64-bit words: what the comment insert takes (tiles, scans, the count, the newline
// index) and one more word per record: where its '+' lies
extern "C" uint64_t scalce_fastq_plus_ws_bytes(uint64_t nrecords, uint64_t entry_bytes) {
  return scalce_fastq_comment_ws_bytes(nrecords, entry_bytes) + sizeof(u64) * (nrecords + 8);
}
static int plus_window(scalce_ctx *c, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets, const uint8_t *d_entries,
                       uint64_t entry_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets, uint32_t *d_bad, void *d_ws, hipStream_t s) {
  u64 *tile = static_cast<u64 *>(d_ws), *scan = tile + comment_ws_tiles(entry_bytes), *nlines = scan + comment_ws_scan(nrecords, entry_bytes);
  u64 *ent_end = nlines + 8, *plus_at = ent_end + nrecords + 8;
  // the newline index of the entries, and the verdict on their count, as the comment insert makes them
  HIP_TRY(c, hipMemsetAsync(nlines, 0, sizeof(u64) * (8 + nrecords), s));
  const u32 ntiles = cdiv(entry_bytes, IDX_TILE);
  if (ntiles) {
    LAUNCH(index_count_k, ntiles, IDX_THREADS, 0, s, d_entries, entry_bytes, tile);
    exclusive_scan<u64>(LoadAs<u64, u64>{tile}, ntiles, StoreTo<u64>{tile}, scan, nlines, s);
    LAUNCH(index_write_k, ntiles, IDX_THREADS, 0, s, d_entries, entry_bytes, tile, ent_end, nrecords);
  }
  LAUNCH(insert_check_k, 1, 1, 0, s, nlines, d_entries, entry_bytes, nrecords, d_bad);
  PlusArgs a;
  a.text = d_text; a.rec_off = reinterpret_cast<const u64 *>(d_record_offsets); a.entries = d_entries; a.entry_bytes = entry_bytes;
  a.ent_end = ent_end; a.nrec = nrecords; a.plus_at = plus_at; a.dst_off = reinterpret_cast<u64 *>(d_out_offsets); a.dst = d_out;
  a.dst_cap = out_cap; a.bad = d_bad;
  if (nrecords) LAUNCH(plus_insert_plan_k, cdiv(nrecords, 256), 256, 0, s, a);
  exclusive_scan<u64>(LoadAs<u64, u64>{a.dst_off}, nrecords, StoreTo<u64>{a.dst_off}, scan, a.dst_off + nrecords, s);
  // (the grid covers the room the caller gave; the workgroups behind the text's end return at once)
  if (nrecords && out_cap) LAUNCH(plus_insert_copy_k, cdiv(out_cap, VL_SPAN), 256, 0, s, a);
  return launch_failed(c);
}
static int plus_window_args(scalce_ctx *c, uint64_t n, const uint8_t *d_text, const uint64_t *d_off, const uint8_t *d_entries, uint64_t entry_bytes,
                            uint8_t *d_out, uint64_t *d_out_off, uint32_t *d_bad, void *d_ws) {
  if (!c || !d_out_off || !d_bad || !d_ws || n > 0x7FFFFFFFull) return SCALCE_ERR_ARG;
  if (n && (!d_text || !d_off || !d_out)) return SCALCE_ERR_ARG;
  if (entry_bytes && !d_entries) return SCALCE_ERR_ARG;
  if (((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_entries & 15)) {
    set_err(c, "plus lines: the window's texts and its entries must be 16-byte aligned");
    return SCALCE_ERR_ARG;
  }
  return SCALCE_OK;
}
extern "C" int scalce_fastq_plus_window(scalce_ctx *c, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets,
                                        const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                        uint32_t *d_bad, void *d_ws, void *stream) {
  if (int rc = plus_window_args(c, nrecords, d_text, d_record_offsets, d_entries, entry_bytes, d_out, d_out_offsets, d_bad, d_ws)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  return plus_window(c, nrecords, d_text, d_record_offsets, d_entries, entry_bytes, d_out, out_cap, d_out_offsets, d_bad, d_ws, s);
}
// The same for an interleaved window: 2 npairs records, mate 1's the even ones, and their entries in that order.  The records'
// own offsets are made from the pairs' (mate 1's record is its header line and 2 read_len[0] + 5 bytes), and the pairs' new
// offsets taken from the records' new ones.
extern "C" uint64_t scalce_fastq_plus_pairs_ws_bytes(uint64_t npairs, uint64_t entry_bytes) {
  return scalce_fastq_plus_ws_bytes(2 * npairs, entry_bytes) + sizeof(u64) * 2 * comment_pairs_words(npairs);
}
extern "C" int scalce_fastq_plus_window_pairs(scalce_ctx *c, const int read_len[2], uint64_t npairs, const uint8_t *d_text,
                                              const uint64_t *d_pair_offsets, const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out,
                                              uint64_t out_cap, uint64_t *d_out_pair_offsets, uint32_t *d_bad, void *d_ws, void *stream) {
  if (!read_len || npairs > 0x3FFFFFFFull) return SCALCE_ERR_ARG;
  for (int m = 0; m < 2; m++) if (read_len[m] <= 0 || read_len[m] > 65535) return SCALCE_ERR_ARG;
  if (int rc = plus_window_args(c, npairs, d_text, d_pair_offsets, d_entries, entry_bytes, d_out, d_out_pair_offsets, d_bad, d_ws)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, hipSetDevice(c->device));
  u64 *rec_off = reinterpret_cast<u64 *>(static_cast<u8 *>(d_ws) + scalce_fastq_plus_ws_bytes(2 * npairs, entry_bytes));
  u64 *new_off = rec_off + comment_pairs_words(npairs);
  LAUNCH(plus_pair_split_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, d_text, reinterpret_cast<const u64 *>(d_pair_offsets), (u64)read_len[0], rec_off);
  const int rc = plus_window(c, 2 * npairs, d_text, reinterpret_cast<const uint64_t *>(rec_off), d_entries, entry_bytes, d_out, out_cap,
                             reinterpret_cast<uint64_t *>(new_off), d_bad, d_ws, s);
  if (rc) return rc;
  LAUNCH(pair_offsets_k, cdiv(npairs + 1, 256), 256, 0, s, npairs, new_off, reinterpret_cast<u64 *>(d_out_pair_offsets));
  return launch_failed(c);
}
