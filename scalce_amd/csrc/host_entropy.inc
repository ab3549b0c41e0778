// host_entropy.inc -- part of scalce_hip.hip (one translation unit; included there, in this order): stage 5: tables, block buffers or coding in place, the coder launches (one job, grouped, windowed), framing, collect, rerun
// ---- stage 5: entropy ---------------------------------------------------------------------------------
// Code one mate's symbol stream `d_sym` (nsym symbols, first symbol = start of a 10 MiB block of the run-wide
// stream) against `table` (device, 512000 x u32, already scaled).
// One coder job = one mate's symbol stream of one shard.  A launch codes the blocks of one or more jobs.
struct AcJob {
  scalce_batch *b;
  int m;
  const u8 *sym;
  u64 nsym;
  u32 nblk;
  bool general;
  u32 max_total = 0;
};
static const u64 AC_STRIDE = (u64)AC_BLOCK_SYMS + 4096;  // the reference's own output buffer is 10 MiB (arithmetic.cpp:301)
constexpr u32 AC_LOG_WORDS = 1024;        // carry notes per block coded in place (a note needs 32 ones in a row in the stream)

// table -> reciprocal fractions, buffers; one short wait for the largest context total
static int ac_prepare(AcJob &j, hipStream_t s, bool framed_output = true, bool full_stride = false, bool allow_in_place = false) {
  scalce_batch *b = j.b;
  scalce_ctx *c = b->ctx;
  const int m = j.m;
  u32 *table = b->table[m].as<u32>();
  ENSURE(b, b->ac_tab[m], sizeof(uint4) * 512000);
  ENSURE(b, b->ac_cum[m], sizeof(u32) * 6400 * 81);
  // one read-back for both: the largest context total and the table's own coding cost
  BatchScratch::TableInfo *tinfo = &b->d_scr->tinfo[m];
  HIP_TRY(c, hipMemsetAsync(tinfo, 0, sizeof *tinfo, s));
  ENSURE(b, b->ac_tab8[m], sizeof(u64) * (6400 * 81 + 2));
  LAUNCH(ac_table_k, cdiv(6400, 64), 64, 0, s, table, b->ac_tab[m].as<uint4>(), b->ac_cum[m].as<u32>(), reinterpret_cast<u32 *>(&tinfo->max_total), b->ac_tab8[m].as<u64>(),
         tinfo->cost);
  BatchScratch::TableInfo th = {0, {0, 0}};
  { int rc = read_words(b, tinfo, &th, sizeof th / 4, s); if (rc) return rc; }
  const u32 max_total = (u32)th.max_total;
  // above 2^30 a symbol's interval can collapse in the reference's 32-bit coder; only the general step
  // follows it there bit for bit
  j.general = max_total > (1u << 30) || getenv("SCALCE_AC_GENERAL") != nullptr;
  j.max_total = max_total;
  j.nblk = (u32)cdiv(j.nsym, AC_BLOCK_SYMS);
  {
    u64 stride = AC_STRIDE;
    const char *scale_env = getenv("SCALCE_AC_STRIDE_SCALE");  // test hook: "0" = the reference's full stride, else a factor (too small on purpose)
    const bool full = scale_env && atof(scale_env) == 0.0;
    if (!full && !full_stride && th.cost[1]) {
      double bytes_per_symbol = (double)th.cost[0] / 256.0 / 8.0 / (double)th.cost[1];
      if (scale_env) bytes_per_symbol *= atof(scale_env);
      const u64 est = (u64)((double)AC_BLOCK_SYMS * bytes_per_symbol * 1.08) + 65536;
      stride = std::min<u64>(AC_STRIDE, (est + 15) & ~15ull);
    }
    b->ac_stride[m] = stride;
  }
  // in place: only the batch's own reordered stream, whole (the kernels of a grouped launch all know how; ac_encode_k does not)
  b->in_place_now[m] = allow_in_place && b->code_in_place && !b->in_place_suspended && !b->qs_in_ws && j.nblk &&
                       j.sym == b->qs(m).as<u8>() && b->qs(m).cap >= j.nsym + 64 + AC_INPLACE_PAD;
  if (b->in_place_now[m]) {
    b->ac_stride[m] = AC_BLOCK_SYMS;
    b->ac_base[m] = b->qs(m).as<u8>();
    ENSURE(b, b->ac_log[m], sizeof(u32) * AC_LOG_WORDS * (size_t)j.nblk + 64);
  } else {
    ENSURE(b, b->ac_blocks[m], (size_t)j.nblk * b->ac_stride[m] + 4096 + 64);  // (the frame kernels read a few words past a block's bytes)
    b->ac_base[m] = b->ac_blocks[m].as<u8>();
  }
  ENSURE(b, b->ac_sizes[m], sizeof(u32) * (j.nblk + 2));
  ENSURE(b, b->ac_off[m], sizeof(u64) * (j.nblk + 2));
  // the framed stream is sized for the worst case (every block at its cap): no size has to come back from the
  // device before the frame kernel can be enqueued
  if (framed_output && !b->frame_on_demand) ENSURE(b, b->out_qual[m], (size_t)j.nblk * (b->ac_stride[m] + 4) + 64);
  ENSURE(b, b->ac_scan, sizeof(u64) * (scan_ws_elems(j.nblk ? j.nblk : 1) + 64));  // (the batch's own: framing runs at collect time,
  if (!j.nblk) b->out_qual_bytes[m] = 0;                                            //  beside another batch's front stages)
  return SCALCE_OK;
}

// The shape of a coder launch -- which kernel runs, how many blocks each workgroup takes, how many lanes of
// ac_encode_lanes_k hold a block -- is decided here and nowhere else:
//
//   launch                                    blocks per workgroup
//   AC_SINGLE     (encode_stream)             SCALCE_AC_BLOCKS_PER_WG if set (4, 8, 64), else 1 = ac_encode_k, one job only
//   AC_PAIRED     (both mates, one launch)    <= 1024 blocks: 4, else 8 (with the override set each mate is an AC_SINGLE launch)
//   AC_RECODE     (entropy_recode_full)       <= 1024: 4, else 8; the override is ignored
//   AC_WINDOW     (entropy_windowed)          8; the override is ignored
//   AC_GROUP(_LAST) (grouped launch)          < 900: 4, else 64; AC_GROUP_LAST with 900 .. 2048 blocks: 8; the override replaces it
//   any launch at 64 that needs the general step: 8 (one block per lane only follows the reference while no interval can
//   invert, kernels_acl.hpp)
//
//   lanes per workgroup (64 only): SCALCE_AC_LANES_USED if set (ac_lanes_override); else AC_GROUP_LAST:
//   clamp(ceil(blocks / CUs), 8, 64), the others 32.
//
//   symbols per round (64 only): rows of up to 48 lanes 32, or SCALCE_AC_ROUND (16 | 32) if set; wider rows 16 (their arrays
//   do not fit into the LDS at 32).  ac_launch runs rows of up to 48 lanes as <48, 3, 32> or <48, 5, 16> --
//   either way the gather wave is 64 symbols ahead of the chain -- and wider ones as <64, 5, 16>.
//
// One block per workgroup has the lowest latency of a block; four take 0.57 x the SIMD time per block at 1.2 x the
// latency.  Paired reads: both mates' streams in ONE launch instead of two launches of the one-block kernel behind each
// other -- the same chip, half the time.  Grouped launches: as few blocks per workgroup as keep the launch at one
// workgroup per CU (256 CUs), so that every chain wave has a SIMD of its own -- one shard (477 blocks at 50 M x 100) at
// four; from two shards on one block per LANE: the launch then takes ~0.56 s whatever its size, but on a sixth of the SIMD
// time per block, and the front stages of the next shards keep the chip (DESIGN.md section 5).  The last launch of a run
// (nothing is queued behind it) is judged by how soon it is done, not by how few CUs it holds: eight blocks per chain wave
// (0.36-0.47 s for up to 2048 blocks) instead of one block per lane (0.56-0.65 s), and one block per lane beyond that on
// every CU with as few blocks per workgroup as that allows (0.45 s at 24, 0.47 at 32, 0.50 at 40).
enum AcLaunchKind { AC_SINGLE, AC_PAIRED, AC_RECODE, AC_WINDOW, AC_GROUP, AC_GROUP_LAST };
struct AcShape {
  int blocks_per_wg;  // 1 = ac_encode_k, 4 / 8 = ac_encode_rows_k, 64 = ac_encode_lanes_k (one block per lane)
  u32 lanes;          // ac_encode_lanes_k: blocks per workgroup
  int round;          // ac_encode_lanes_k: symbols per block and round (16 or 32)
};

// SCALCE_AC_BLOCKS_PER_WG (tests, tools/coder_alone.py): 4, 8 or 64; 0 = no override
static int ac_blocks_override() {
  const char *e = getenv("SCALCE_AC_BLOCKS_PER_WG");
  const int v = e ? atoi(e) : 0;
  return (v == 4 || v == 8 || v == 64) ? v : 0;
}

// Blocks per workgroup of ac_encode_lanes_k.  A lane per block would be 64; the default is fewer: all table rows of a
// workgroup's blocks go through ONE CU's vector memory pipeline (1024 scattered 16-byte reads per 0.75 us round at 64), and
// beside another shard's streaming front stages -- when an L2 miss takes three times as long -- that pipeline, not the coder,
// set the pace of a launch: 908 ms beside the ingest stage and 1299 ms beside the order stage at 64 blocks per workgroup
// against 575 / 694 ms at 32 and 560 / 559 ms at 16 (543 ms alone; DESIGN_HISTORY.md).  Fewer blocks per workgroup
// are more CUs held per launch, CUs the front stages of the next shards do not get: in round 3's mix 48 was the best
// trade (ms per shard at 32 / 40 / 48 / 56 / 64 blocks: 107.0 / 106.6 / 102.4 / 108.0 / 115.5; DESIGN.md section 7).
// Round 4 (twelve slots, block buffers of their own): 79.9 / 80.0 / 81.1 / 81.7 / 82.2 / 85.6 ms per shard at 32 / 36 / 40 /
// 44 / 48 / 56, 40 the default.  Round 5 (fifteen slots, coded in place, six shards per launch on two streams;
// tools/r5_sweep.sh): 79.3 / 79.6 / 74.0 / 74.6 / 75.2 / 77.9 / 81.8 at 24 / 28 / 32 / 36 / 40 / 48 / 56 -- a launch takes
// 0.47 s at 32 against 0.50 at 40, and with slots to spare the pipeline follows the launch's latency: 32.
// SCALCE_AC_LANES_USED overrides it (1 .. 64; anything else is 32); 0 = not set.
static u32 ac_lanes_override() {
  const char *e = getenv("SCALCE_AC_LANES_USED");
  if (!e) return 0;
  const int v = atoi(e);
  return (u32)(v < 1 || v > 64 ? 32 : v);
}

// Symbols per round of ac_encode_lanes_k for rows of up to 48 lanes: SCALCE_AC_ROUND = 16 or 32 (tests, measurements; the
// same bytes either way); 0 = not set or anything else.
static int ac_round_override() {
  const char *e = getenv("SCALCE_AC_ROUND");
  const int v = e ? atoi(e) : 0;
  return v == 16 || v == 32 ? v : 0;
}
constexpr int AC_ROUND_DEFAULT = 32;  // (measured: DESIGN.md section 5)

static AcShape ac_shape(AcLaunchKind kind, u32 blocks, bool general, int device) {
  const int over = ac_blocks_override();
  int bpw;
  switch (kind) {
    case AC_SINGLE: bpw = over ? over : 1; break;
    case AC_PAIRED:
    case AC_RECODE: bpw = blocks <= 1024 ? 4 : 8; break;
    case AC_WINDOW: bpw = 8; break;
    default:
      bpw = blocks < 900 ? 4 : (kind == AC_GROUP_LAST && blocks <= 2048) ? 8 : 64;
      if (over) bpw = over;
  }
  if (bpw == 64 && general) bpw = 8;
  u32 lanes = ac_lanes_override();
  if (!lanes && kind == AC_GROUP_LAST && bpw == 64) {
    static int n_cus = 0;
    if (!n_cus) { hipDeviceProp_t pr; n_cus = hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
    lanes = std::min<u32>(std::max<u32>(cdiv(blocks, (u32)n_cus), 8u), 64u);
  }
  if (!lanes) lanes = 32u;
  return AcShape{bpw, lanes, lanes <= 48 ? (ac_round_override() ? ac_round_override() : AC_ROUND_DEFAULT) : 16};
}

// ONE launch over the blocks of all jobs, in the shape ac_shape gives `kind`.
// `ps` = the stream the tables were prepared on: the block descriptors are uploaded there (never behind a coder that
// is still running on `s`), and `s` is made to wait for it.
static int ac_launch(AcJob *jobs, int njobs, AcLaunchKind kind, hipStream_t s, hipStream_t ps) {
  scalce_batch *lead = jobs[0].b;
  scalce_ctx *c = lead->ctx;
  u32 total = 0;
  bool general = false;
  for (int i = 0; i < njobs; i++) {
    total += jobs[i].nblk;
    general |= jobs[i].general;
    // the plain path's exit test (see ac_encode_k) needs every symbol to keep an interval of two values or more
    if (jobs[i].max_total > (1u << 29)) general = true;
  }
  if (!total) return SCALCE_OK;
  const AcShape shape = ac_shape(kind, total, general, c->device);
  AcEncArgs a;
  memset(&a, 0, sizeof a);
  a.slow_threshold = 32;
  a.chain_prio = 3u;
  a.helper_prio = 0u;
  a.test_poison = getenv("SCALCE_AC_TEST_POISON") ? (u32)atoi(getenv("SCALCE_AC_TEST_POISON")) : 0u;  // test hook
  a.inplace_shift = getenv("SCALCE_AC_INPLACE_TEST") ? 2u : 0u;  // test hook: a block coded in place catches up with its input
  a.simd_load = c->d_simd_load.as<u32>();
  if (const char *e = getenv("SCALCE_AC_SLOW_THRESHOLD")) a.slow_threshold = (u32)atoi(e);  // test hook
  auto join = [&]() -> int {  // `s` continues behind everything enqueued on `ps` so far
    if (ps == s) return SCALCE_OK;
    hipEvent_t ev = lead->ev_group;
    if (!ev) { HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming)); lead->ev_group = ev; }
    HIP_TRY(c, hipEventRecord(ev, ps));
    HIP_TRY(c, hipStreamWaitEvent(s, ev, 0));
    return SCALCE_OK;
  };
  hipEvent_t ke0 = nullptr, ke1 = nullptr;
  if (lead->ktiming) {
    if (lead->kev_used == lead->kev.size()) {
      hipEvent_t x, y;
      HIP_TRY(c, hipEventCreate(&x));
      HIP_TRY(c, hipEventCreate(&y));
      lead->kev.emplace_back(x, y);
    }
    ke0 = lead->kev[lead->kev_used].first; ke1 = lead->kev[lead->kev_used].second;
    lead->kev_used++;
  }
  if (shape.blocks_per_wg == 1) {
    if (njobs != 1) { set_err(c, "internal: ac_encode_k takes one job"); return SCALCE_ERR_ARG; }
    scalce_batch *b = jobs[0].b;
    const int m = jobs[0].m;
    a.sym = jobs[0].sym; a.nsym = jobs[0].nsym; a.tab = b->ac_tab[m].as<uint4>(); a.out = b->ac_base[m];
    a.out_stride = b->ac_stride[m]; a.out_cap = (u32)b->ac_stride[m]; a.out_size = b->ac_sizes[m].as<u32>(); a.err = b->d_err;
    { int rc = join(); if (rc) return rc; }
    if (ke0) hipEventRecord(ke0, s);
    if (general) LAUNCH(ac_encode_k<true>, total, 128, 0, s, a);
    else LAUNCH(ac_encode_k<false>, total, 128, 0, s, a);
    if (ke1) hipEventRecord(ke1, s);
  } else {
    // block descriptors: the launch may hold blocks of several shards, each with its own table and output
    if (total > lead->ac_desc_cap) {
      if (lead->ac_desc_host) hipHostFree(lead->ac_desc_host);
      lead->ac_desc_host = nullptr;
      lead->ac_desc_cap = 0;
      // (room for any launch this shard is likely to lead: an allocation synchronises the whole device -- a shard that led a
      //  launch of one shard and then one of three waited there for every coder that was running)
      const u32 cap = std::max<u32>(total + total / 2, 8192u);
      HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&lead->ac_desc_host), sizeof(AcBlockDesc) * (size_t)cap, hipHostMallocDefault));
      lead->ac_desc_cap = cap;
    }
    const bool lanes = shape.blocks_per_wg == 64;  // gathers from the compact table
    AcBlockDesc *d = lead->ac_desc_host;
    u32 nd = 0;
    for (int i = 0; i < njobs; i++) {
      scalce_batch *b = jobs[i].b;
      const int m = jobs[i].m;
      for (u32 k = 0; k < jobs[i].nblk; k++) {
        AcBlockDesc x;
        const u64 off = (u64)k * AC_BLOCK_SYMS;
        x.sym = jobs[i].sym + off;
        x.tab = lanes ? reinterpret_cast<const uint4 *>(b->ac_tab8[m].as<u64>()) : b->ac_tab[m].as<uint4>();
        x.dst = reinterpret_cast<u32 *>(b->ac_base[m] + (u64)k * b->ac_stride[m]);
        x.cap = (u32)b->ac_stride[m];
        x.flags = 0; x.log = nullptr; x.log_cap = 0; x.pad_ = 0;
        if (b->in_place_now[m]) {   // the block's own symbols are its buffer; the last block of a stream may run into the padding
          const u64 left = jobs[i].nsym - (u64)k * AC_BLOCK_SYMS;
          if (left < AC_BLOCK_SYMS) x.cap = (u32)std::min<u64>(AC_BLOCK_SYMS, (left + AC_INPLACE_PAD) & ~3ull);
          x.flags = AC_BLOCK_IN_PLACE;
          x.log = b->ac_log[m].as<u32>() + (size_t)k * AC_LOG_WORDS;
          x.log_cap = AC_LOG_WORDS;
        }
        x.out_size = b->ac_sizes[m].as<u32>() + k;
        x.err = b->d_err;
        x.n = (u32)std::min<u64>(AC_BLOCK_SYMS, jobs[i].nsym - off);
        x.index = k;
        d[nd++] = x;
      }
    }
    ENSURE(lead, lead->ac_desc, sizeof(AcBlockDesc) * (size_t)lead->ac_desc_cap);
    HIP_TRY(c, hipMemcpyAsync(lead->ac_desc.p, d, sizeof(AcBlockDesc) * total, hipMemcpyHostToDevice, ps));
    a.desc = lead->ac_desc.as<AcBlockDesc>();
    a.nblocks = total;
    a.out_cap = (u32)AC_STRIDE;
    { int rc = join(); if (rc) return rc; }
    if (ke0) hipEventRecord(ke0, s);
    if (lanes) {
      a.lanes_used = shape.lanes;
      // (two sets of four waves per CU -- a chain or sink sharing its SIMD with a light wave of the other set -- cost a third fewer
      //  CU-seconds and 35 % more latency per launch: 98 against 75 ms per shard with fifteen slots, round 5; waves on shared CUs at
      //  raised priority: +5 %, round 3.  Both removed.)
      lead->ac_round_launched = shape.round;  // (scalce_batch_coder_round: tests)
      if (a.lanes_used <= 48 && shape.round == 32) LAUNCH((ac_encode_lanes_k<48, 3, 32>), cdiv(total, a.lanes_used), 256, 0, s, a);
      else if (a.lanes_used <= 48) LAUNCH((ac_encode_lanes_k<48, 5, 16>), cdiv(total, a.lanes_used), 256, 0, s, a);  // (rows of 48: LDS for a longer staging ring)
      else LAUNCH((ac_encode_lanes_k<64, 5, 16>), cdiv(total, a.lanes_used), 256, 0, s, a);
    } else if (shape.blocks_per_wg == 8) {
      if (general) LAUNCH((ac_encode_rows_k<true, 8>), cdiv(total, 8), 320, 0, s, a);
      else LAUNCH((ac_encode_rows_k<false, 8>), cdiv(total, 8), 320, 0, s, a);
    } else {
      if (general) LAUNCH((ac_encode_rows_k<true, 16>), cdiv(total, 4), 192, 0, s, a);
      else LAUNCH((ac_encode_rows_k<false, 16>), cdiv(total, 4), 192, 0, s, a);
    }
    if (ke1) hipEventRecord(ke1, s);
  }
  for (int i = 0; i < njobs; i++) {
    lead->k_in_bytes += jobs[i].nsym;
    jobs[i].b->ac_last_sym[jobs[i].m] = jobs[i].sym;
    jobs[i].b->ac_last_nsym[jobs[i].m] = jobs[i].nsym;
  }
  return SCALCE_OK;
}

// framing: sizes -> offsets -> [u32 size][bytes] per block, all enqueued; the total is read back by entropy_collect
static int ac_frame(AcJob &j, hipStream_t s) {
  scalce_batch *b = j.b;
  const int m = j.m;
  b->frame_virtual[m] = 0;
  if (!j.nblk) return SCALCE_OK;
  exclusive_scan<u64>(AcFrameLen{b->ac_sizes[m].as<u32>()}, j.nblk, StoreTo<u64>{b->ac_off[m].as<u64>()}, b->ac_scan.as<u64>(),
                      &b->d_scr->frame_bytes[m], s);
  if (b->frame_on_demand) {  // the layout is all there is for now
    b->frame_virtual[m] = j.nblk;
    b->ent_pending[m] = j.nblk;
    return SCALCE_OK;
  }
  if (b->out_qual[m].cap < (size_t)j.nblk * (b->ac_stride[m] + 4) + 64) {
    // the framed stream was not sized for the worst case (a grouped launch: twelve and more shards in flight, and 5 GB each
    // of a capacity that is little more than half used is a shard less in flight): the size comes back first -- the coder has
    // finished, this is a wait of microseconds -- and the buffer grows when a shard codes worse than any before it
    u64 total = 0;
    { int rc = read_u64(b, &b->d_scr->frame_bytes[m], &total, 1, s); if (rc) return rc; }
    if (b->out_qual[m].cap < total + 64) ENSURE(b, b->out_qual[m], (size_t)(total + total / 16) + (32u << 20));
  }
  LAUNCH(ac_frame_k, dim3(cdiv(b->ac_stride[m], 16 * 256), j.nblk), 256, 0, s, b->ac_base[m], b->ac_stride[m],
         b->ac_sizes[m].as<u32>(), b->ac_off[m].as<u64>(), b->out_qual[m].as<u8>());
  b->ent_pending[m] = j.nblk;
  return SCALCE_OK;
}

// Code one mate's symbol stream `d_sym` (nsym symbols, first symbol = start of a 10 MiB block of the run-wide
// stream) against `table` (device, 512000 x u32, already scaled).
static int encode_stream(scalce_batch *b, int m, const u8 *d_sym, u64 nsym, hipStream_t s) {
  AcJob j{b, m, d_sym, nsym, 0, false};
  int rc = ac_prepare(j, s);
  if (rc) return rc;
  if ((rc = ac_launch(&j, 1, AC_SINGLE, s, s))) return rc;
  return ac_frame(j, s);
}

// A block outgrew the stride its shard's table suggested (ac_prepare): the shard's streams are coded again with the
// reference's own 10 MiB per block, now, on the collecting stream.  Rare by construction; the same bytes one launch later.
static int entropy_recode_full(scalce_batch *b, hipStream_t s) {
  std::vector<AcJob> jobs;
  for (int m = 0; m < b->nm; m++) {
    if (!b->ac_last_sym[m] || !b->ac_last_nsym[m]) continue;
    AcJob j{b, m, b->ac_last_sym[m], b->ac_last_nsym[m], 0, false};
    int rc = ac_prepare(j, s, /*framed_output=*/false, /*full_stride=*/true);
    if (rc) return rc;
    jobs.push_back(j);
  }
  if (jobs.empty()) return SCALCE_OK;
  int rc = ac_launch(jobs.data(), (int)jobs.size(), AC_RECODE, s, s);
  if (rc) return rc;
  for (auto &j : jobs) { b->frame_deferred[j.m] = j.nblk; b->ent_pending[j.m] = 0; }
  return SCALCE_OK;
}

// A block coded in place caught up with its own input (kernels_acl.hpp, writer wave; kernels_ac.hpp, helper waves): the symbols
// it had consumed are under its output, nothing can be coded again from them.  The shard is run again from its TEXT -- which a
// caller that turns coding in place on keeps where it was until the shard is collected -- with block buffers of its own.
// Never seen on quality strings (their code is shorter than their symbols by a third and more from the first round on);
// SCALCE_AC_INPLACE_TEST=1 makes the kernels' bound so tight that it happens (tests).
static int entropy_rerun_from_text(scalce_batch *b, hipStream_t s) {
  scalce_ctx *c = b->ctx;
  if (b->appending || b->base != 0 || !b->piece_text[0] || (b->nm == 2 && !b->piece_text[1])) {
    set_err(c, "a block coded in place outgrew its input and the shard's text is not at hand to run it again (scalce_batch_set_code_in_place)");
    return SCALCE_ERR_CAPACITY;
  }
  static const bool dbg = getenv("SCALCE_TRACE") != nullptr;
  if (dbg) fprintf(stderr, "scalce: batch %p: a block coded in place caught up with its input: the shard is run again from its text\n", (void *)b);
  const u8 *t1 = b->piece_text[0], *t2 = b->ntext == 2 ? b->piece_text[1] : nullptr;
  const u64 n1 = b->text_bytes[0], n2 = b->ntext == 2 ? b->text_bytes[1] : 0;
  for (int m = 0; m < 2; m++) { b->frame_deferred[m] = 0; b->ent_pending[m] = 0; b->in_place_now[m] = false; }
  b->in_place_suspended = true;
  b->reruns++;
  int rc = scalce_batch_front(b, t1, n1, t2, n2, s);
  if (!rc) rc = scalce_batch_entropy(b, nullptr, s);
  b->in_place_suspended = false;
  return rc;
}

// second half of the entropy stage: wait for the coder and read the size of the framed stream(s)
static int entropy_collect(scalce_batch *b, hipStream_t s) {
  {
    bool open = false, tight = false, in_place = false;
    for (int m = 0; m < b->nm; m++) {
      open |= b->frame_deferred[m] != 0 || b->ent_pending[m] != 0;
      tight |= b->ac_stride[m] != 0 && b->ac_stride[m] < AC_STRIDE;
      in_place |= b->in_place_now[m];
    }
    if (open && tight) {
      DevErr e;
      HIP_TRY(b->ctx, hipMemcpyAsync(&e, b->d_err, sizeof e, hipMemcpyDeviceToHost, s));
      HIP_TRY(b->ctx, hipStreamSynchronize(s));
      if (e.code == E_ACOVERFLOW) {
        if (getenv("SCALCE_TRACE"))
          fprintf(stderr, "scalce: batch %p: block %llu outgrew its %llu-byte buffer (it needed %u): coding the shard again at the full stride\n",
                  (void *)b, (unsigned long long)e.where, (unsigned long long)b->ac_stride[0], e.aux);
        HIP_TRY(b->ctx, hipMemsetAsync(b->d_err, 0, sizeof(DevErr), s));
        if (in_place) return entropy_rerun_from_text(b, s);   // (collects by itself)
        int rc = entropy_recode_full(b, s);
        if (rc) return rc;
      }
    }
  }
  for (int m = 0; m < b->nm; m++) {
    if (b->frame_deferred[m]) {
      AcJob j{b, m, nullptr, 0, b->frame_deferred[m], false};
      b->frame_deferred[m] = 0;
      int rc = ac_frame(j, s);
      if (rc) return rc;
    }
    if (!b->ent_pending[m]) continue;
    u64 total = 0;
    if (b->frame_virtual[m]) {  // (one wait for both: the layout and the total)
      b->frame_off_host[m].resize(b->frame_virtual[m]);
      HIP_TRY(b->ctx, hipMemcpyAsync(b->frame_off_host[m].data(), b->ac_off[m].p, sizeof(u64) * b->frame_virtual[m], hipMemcpyDeviceToHost, s));
    }
    { int rc = read_u64(b, &b->d_scr->frame_bytes[m], &total, 1, s); if (rc) return rc; }
    b->out_qual_bytes[m] = total;
    b->k_out_bytes += total - 4ull * b->ent_pending[m];
    b->ent_pending[m] = 0;
  }
  return SCALCE_OK;
}

// table of one mate: the shard's own statistics, scaled (compress.cpp:297-303), or the caller's run-wide table
static int ac_table_for(scalce_batch *b, int m, const uint32_t *d_table_override, u64 nsym, hipStream_t s) {
  scalce_ctx *c = b->ctx;
  u32 *table = b->table[m].as<u32>();
  if (d_table_override) {
    HIP_TRY(c, hipMemcpyAsync(table, d_table_override + (size_t)m * 512000, sizeof(u32) * 512000, hipMemcpyDeviceToDevice, s));
  } else {
    const u32 factor = 1 + (u32)(nsym / 0xFFFFFFFFull);  // compress.cpp:297-303
    LAUNCH(ac_scale_k, cdiv(512000, 256), 256, 0, s, b->freq4[m].as<u64>(), factor, table);
  }
  return SCALCE_OK;
}

// Runs with more blocks than a launch should hold (200 M x 150 bp paired: 5 724): the streams are coded window by window --
// up to AC_WINDOW_BLOCKS blocks per launch over both mates -- into block buffers sized for one window, and every window
// is framed straight behind the previous one.  Sized for the worst case as the one-launch path does, the buffers of
// such a run would take 2 x 60 GB per mate.
constexpr u32 AC_WINDOW_BLOCKS = 2048;  // 256 workgroups of eight
static int entropy_windowed(scalce_batch *b, const uint32_t *d_table_override, hipStream_t s) {
  scalce_ctx *c = b->ctx;
  const u64 N = b->N;
  u32 W = AC_WINDOW_BLOCKS / (u32)b->nm;
  if (const char *e = getenv("SCALCE_AC_WINDOW_BLOCKS")) W = (u32)std::max(1, atoi(e));  // test hook: blocks per mate and window
  u64 used[2] = {0, 0}, nsym[2] = {0, 0};
  u32 nblk[2] = {0, 0}, most = 0;
  for (int m = 0; m < b->nm; m++) {
    nsym[m] = N * (u64)b->L[m];
    nblk[m] = cdiv(nsym[m], AC_BLOCK_SYMS);
    most = nblk[m] > most ? nblk[m] : most;
    b->frame_virtual[m] = 0;   // this path writes the framed stream itself: a layout left by an earlier shard is void
    b->frame_off_host[m].clear();
    int rc = ac_table_for(b, m, d_table_override, nsym[m], s);
    if (rc) return rc;
    b->out_qual_bytes[m] = 0;
  }
  bool first = true;
  for (u32 w0 = 0; w0 < most; w0 += W) {
    AcJob jobs[2];
    int nj = 0;
    for (int m = 0; m < b->nm; m++) {
      if (w0 >= nblk[m]) continue;
      const u64 off = (u64)w0 * AC_BLOCK_SYMS;
      const u64 n = std::min<u64>(nsym[m] - off, (u64)W * AC_BLOCK_SYMS);
      jobs[nj] = AcJob{b, m, b->qs(m).as<u8>() + off, n, 0, false};
      int rc = ac_prepare(jobs[nj], s, /*framed_output=*/false, /*full_stride=*/true);  // (windows are collected as they go: no second try)
      if (rc) return rc;
      nj++;
    }
    if (!nj) break;
    int rc = ac_launch(jobs, nj, AC_WINDOW, s, s);
    if (rc) return rc;
    for (int i = 0; i < nj; i++) {
      const int m = jobs[i].m;
      exclusive_scan<u64>(AcFrameLen{b->ac_sizes[m].as<u32>()}, jobs[i].nblk, StoreTo<u64>{b->ac_off[m].as<u64>()}, b->ac_scan.as<u64>(),
                          &b->d_scr->frame_bytes[m], s);
      u64 total = 0;
      if ((rc = read_u64(b, &b->d_scr->frame_bytes[m], &total, 1, s))) return rc;
      if (first) {  // size the framed stream from the first window's ratio; it grows if a later window codes worse
        const u64 est = (u64)((double)total / (double)jobs[i].nsym * 1.03 * (double)nsym[m]) + (64u << 20);
        ENSURE(b, b->out_qual[m], est);
      }
      if ((rc = ensure_keep(b, b->out_qual[m], used[m] + total + 64, used[m], s))) return rc;
      LAUNCH(ac_frame_k, dim3(cdiv(b->ac_stride[m], 16 * 256), jobs[i].nblk), 256, 0, s, b->ac_base[m], b->ac_stride[m],
             b->ac_sizes[m].as<u32>(), b->ac_off[m].as<u64>(), b->out_qual[m].as<u8>() + used[m]);
      used[m] += total;
      b->k_out_bytes += total - 4ull * jobs[i].nblk;
    }
    first = false;
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  for (int m = 0; m < b->nm; m++) { b->out_qual_bytes[m] = used[m]; b->ent_pending[m] = 0; }
  return SCALCE_OK;
}

extern "C" int scalce_batch_entropy_begin(scalce_batch *b, const uint32_t *d_table_override, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  if (b->nq) {  // -Q / -f: no quality stream, nothing to code (SCALCE_OUT_QUAL is empty)
    for (int m = 0; m < b->nm; m++) b->out_qual_bytes[m] = 0;
    return SCALCE_OK;
  }
  const u64 N = b->N;
  if (!b->p.no_ac) {
    u64 blocks = 0;
    for (int m = 0; m < b->nm; m++) blocks += cdiv(N * (u64)b->L[m], AC_BLOCK_SYMS);
    if (blocks > AC_WINDOW_BLOCKS || getenv("SCALCE_AC_WINDOW_BLOCKS")) return entropy_windowed(b, d_table_override, s);  // (the variable: a test hook)
  }
  if (b->nm == 2 && !b->p.no_ac && !ac_blocks_override()) {  // paired reads: both mates' streams in ONE launch (ac_shape)
    AcJob jobs[2];
    for (int m = 0; m < 2; m++) {
      const u64 nsym = N * (u64)b->L[m];
      int rc = ac_table_for(b, m, d_table_override, nsym, s);
      if (rc) return rc;
      jobs[m] = AcJob{b, m, b->qs(m).as<u8>(), nsym, 0, false};
      if ((rc = ac_prepare(jobs[m], s))) return rc;
    }
    int rc = ac_launch(jobs, 2, AC_PAIRED, s, s);
    if (rc) return rc;
    for (int m = 0; m < 2; m++)
      if ((rc = ac_frame(jobs[m], s))) return rc;
    return SCALCE_OK;
  }
  for (int m = 0; m < b->nm; m++) {
    const u64 nsym = N * (u64)b->L[m];
    if (b->p.no_ac) {  // -A: raw q' bytes (compress.cpp:389-390)
      b->out_qual_bytes[m] = nsym;
      continue;
    }
    int rc = ac_table_for(b, m, d_table_override, nsym, s);
    if (rc) return rc;
    if ((rc = encode_stream(b, m, b->qs(m).as<u8>(), nsym, s))) return rc;
  }
  return SCALCE_OK;
}

// Several shards, ONE coder launch (four blocks per workgroup): a shard of 477 blocks fills 120 workgroups, so
// the blocks of two shards fit the 256 CUs one workgroup each -- every chain wave gets a SIMD of its own by
// construction, which two separate launches cannot guarantee (the dispatcher places waves without knowing their
// role; where two chains meet the younger one starves).  Tables are prepared on `prep_stream` (the caller's front
// stream: the host waits there for each table's largest context total, never behind a running coder); coder and
// framing are enqueued on `stream` behind that.  Shards that called scalce_batch_entropy_stream_prepare code the
// stream they were given, the others their own reordered stream.
extern "C" int scalce_batch_entropy_begin_group(scalce_batch **bs, int n, void *prep_stream, void *stream) {
  return scalce_batch_entropy_begin_group_last(bs, n, prep_stream, stream, 0);
}
// last = 1: nothing will be queued behind this launch (the end of a run, or a wave of shards behind whose front stages
// nothing is waiting); 0: more shards follow (ac_shape).  The framing ([u32 size][bytes] per block: a scan of the sizes +
// one copy kernel, ~1.5 ms per 50 M-read shard on an idle chip) is left to entropy_collect, i.e. to the stream the caller
// collects on: behind the coder on its own stream it was measured slower with one coder stream (it lengthens the launch
// the pipeline waits for) and with three (95.6 against 93.0 ms per shard).
extern "C" int scalce_batch_entropy_begin_group_last(scalce_batch **bs, int n, void *prep_stream, void *stream, int last) {
  if (!bs || n <= 0 || n > SCALCE_GROUP_MAX || (last != 0 && last != 1)) return SCALCE_ERR_ARG;
  for (int i = 0; i < n; i++) if (!bs[i] || bs[i]->ctx != bs[0]->ctx) return SCALCE_ERR_ARG;
  hipStream_t ps = (hipStream_t)prep_stream, s = (hipStream_t)stream;
  scalce_ctx *c = bs[0]->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<AcJob> jobs;
  for (int i = 0; i < n; i++) {
    scalce_batch *b = bs[i];
    for (int m = 0; m < b->nm; m++) {
      const u64 own = b->N * (u64)b->L[m];
      if (b->nq) { b->out_qual_bytes[m] = 0; continue; }  // (-Q / -f: nothing to code)
      if (b->p.no_ac) { b->out_qual_bytes[m] = own; continue; }
      AcJob j{b, m, b->ent_external[m] ? b->ent_sym[m] : b->qs(m).as<u8>(), b->ent_external[m] ? b->ent_nsym[m] : own, 0, false};
      if (!b->ent_external[m]) { int rc = ac_table_for(b, m, nullptr, own, ps); if (rc) return rc; }
      b->ent_external[m] = false;
      int rc = ac_prepare(j, ps, /*framed_output=*/false, /*full_stride=*/false, /*allow_in_place=*/true);
      if (rc) return rc;
      jobs.push_back(j);
    }
  }
  if (jobs.empty()) return SCALCE_OK;
  int rc = ac_launch(jobs.data(), (int)jobs.size(), last ? AC_GROUP_LAST : AC_GROUP, s, ps);
  if (rc) return rc;
  for (auto &j : jobs) j.b->frame_deferred[j.m] = j.nblk;
  return SCALCE_OK;
}

// Sharded runs, grouped launch: remember the caller-assembled range of the run-wide stream and its table; the next
// scalce_batch_entropy_begin_group codes it.
extern "C" int scalce_batch_entropy_stream_prepare(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                                   uint64_t nsym, void *stream) {
  if (!b || mate < 0 || mate >= b->nm || !d_table || (nsym && !d_symbols) || b->p.no_ac || b->nq) return SCALCE_ERR_ARG;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(b->table[mate].p, d_table, sizeof(u32) * 512000, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  b->ent_sym[mate] = d_symbols;
  b->ent_nsym[mate] = nsym;
  b->ent_external[mate] = true;
  return SCALCE_OK;
}

extern "C" int scalce_batch_entropy_end(scalce_batch *b, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
  return entropy_collect(b, (hipStream_t)stream);
}

extern "C" int scalce_batch_entropy(scalce_batch *b, const uint32_t *d_table_override, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  if (b->nq) return scalce_batch_entropy_begin(b, d_table_override, stream);  // (-Q / -f: no launch, not even a timed stage)
  StageTimer tm(b, ST_ENTROPY, (hipStream_t)stream);
  int rc = scalce_batch_entropy_begin(b, d_table_override, stream);
  if (rc) return rc;
  return entropy_collect(b, (hipStream_t)stream);
}

// Sharded runs: code `nsym` symbols of mate `mate` that the caller assembled on the device (a range of the
// run-wide reordered stream that starts on a 10 MiB block boundary) against the run-wide table.
extern "C" int scalce_batch_entropy_stream_begin(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                                 uint64_t nsym, void *stream) {
  if (!b || mate < 0 || mate >= b->nm || !d_table || (nsym && !d_symbols) || b->p.no_ac || b->nq) return SCALCE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  scalce_ctx *c = b->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(b->table[mate].p, d_table, sizeof(u32) * 512000, hipMemcpyDeviceToDevice, s));
  return encode_stream(b, mate, d_symbols, nsym, s);
}
extern "C" int scalce_batch_entropy_stream(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                           uint64_t nsym, void *stream) {
  if (!b) return SCALCE_ERR_ARG;
  StageTimer tm(b, ST_ENTROPY, (hipStream_t)stream);
  int rc = scalce_batch_entropy_stream_begin(b, mate, d_table, d_symbols, nsym, stream);
  if (rc) return rc;
  return entropy_collect(b, (hipStream_t)stream);
}

extern "C" int scalce_ac_scale(scalce_ctx *c, const uint64_t *d_counters, uint32_t factor, uint32_t *d_table, void *stream) {
  if (!c || !d_counters || !d_table || !factor) return SCALCE_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  LAUNCH(ac_scale_k, cdiv(512000, 256), 256, 0, (hipStream_t)stream, reinterpret_cast<const u64 *>(d_counters), factor, d_table);
  return SCALCE_OK;
}

// dst[piece_dst[p] + i] = src[piece_src[p] + i] for i < piece_len[p]; pieces sorted by piece_src, contiguous in src
extern "C" int scalce_copy_pieces(scalce_ctx *c, const uint8_t *d_src, uint8_t *d_dst, const uint64_t *d_piece_src,
                                  const uint64_t *d_piece_dst, uint32_t npieces, uint64_t total_bytes, void *stream) {
  if (!c) return SCALCE_ERR_ARG;
  if (!npieces || !total_bytes) return SCALCE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  LAUNCH(copy_pieces_k, cdiv(total_bytes + 15, 256 * 16 * CP_CHUNKS), 256, 0, (hipStream_t)stream, d_src, d_dst,
         reinterpret_cast<const u64 *>(d_piece_src), reinterpret_cast<const u64 *>(d_piece_dst), npieces, (u64)total_bytes);
  return SCALCE_OK;
}
