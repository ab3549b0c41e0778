/*
 * scalce_hip.h -- C ABI of the MI355X (gfx950) SCALCE hot path.
 *
 * The reference (sfu-compbio/scalce 2.8) has no plugin / FFI seam: it is one executable with
 * global state, and its hot path is a set of per-read calls made from thread()
 * (compress.cpp:673-706) and per-stream calls made from the final writer
 * (compress.cpp:296-335,380-391,411-412).  Per-read signatures cannot be driven from a GPU,
 * so every entry point below is the BATCHED equivalent of the reference functions it names.
 * Plain C types, caller-visible integer status, no global state, one context per device.
 *
 * Pointers whose name starts with d_ are DEVICE pointers (HBM); `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  All calls are asynchronous on `stream`
 * unless stated otherwise; scalce_batch_finish() synchronises and reports device-side errors.
 */
#ifndef SCALCE_HIP_H
#define SCALCE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCALCE_OK 0
#define SCALCE_ERR_ARG 1       /* bad argument / state */
#define SCALCE_ERR_HIP 2       /* HIP runtime failure (message in scalce_last_error) */
#define SCALCE_ERR_FORMAT 3    /* malformed input: the cases where the reference prints (ERROR) and exits */
#define SCALCE_ERR_CAPACITY 4  /* batch larger than the capacity it was created with */
/* (5 was SCALCE_ERR_UNCUT in rounds 1-3: a run that -B does not cut is one spill chunk and goes to rank 0 as a whole) */

#define SCALCE_AC_DEPTH 80                  /* arithmetic.h:47 */
#define SCALCE_AC_BLOCK (10 * 1024 * 1024)  /* arithmetic.cpp:48 */
#define SCALCE_ROOT_CORE 0x3FFFFFFF         /* MAXBIN-1: const.h:95, reads.cpp:161-164 */

typedef struct scalce_ctx scalce_ctx;
typedef struct scalce_batch scalce_batch;

/* ---- context ---------------------------------------------------------------------------- */
int scalce_ctx_create(int device, scalce_ctx **out);
void scalce_ctx_destroy(scalce_ctx *ctx);
const char *scalce_last_error(const scalce_ctx *ctx);

/* ---- core table: read_patterns (reads.cpp:330-377), read_patterns_from_file (:379-410),
 *      pattern_insert (:253-267), prepare_aho_automata (:270-324).  Built on the host,
 *      uploaded as a BFS-ordered DFA (state id == the reference's BFS `id`, root 0). ------- */
int scalce_patterns_load_bin(scalce_ctx *ctx, const void *blob, size_t nbytes);
int scalce_patterns_load_text(scalce_ctx *ctx, const char *text, size_t nbytes);
int scalce_patterns_count(const scalce_ctx *ctx);   /* cores in file order (the index .scalcer stores) */
int scalce_patterns_states(const scalce_ctx *ctx);  /* automaton states, root included */
int scalce_patterns_buckets(const scalce_ctx *ctx); /* distinct cores = buckets, root excluded */
/* The tokenizer walk the loaded table selects (decided from the table alone when it is loaded):
 *   SCALCE_WALK_KMER     k-mer tables of the states of depth <= 8 (tokenize_kmer_pipe_k), no core under 8 bases
 *   SCALCE_WALK_KMER_T7  the same, some core has fewer than 8 bases
 *   SCALCE_WALK_ANCHOR   anchors of K = min(shortest core, 12) bases (tokenize_anchor_k); *anchor_k = K
 * SCALCE_WALK_NONE without a table.  *anchor_k (may be null) is 0 unless the walk is SCALCE_WALK_ANCHOR.
 * (4 was the walk of the automaton alone, state by state: no table the loaders accept selected it.) */
#define SCALCE_WALK_NONE 0
#define SCALCE_WALK_KMER 1
#define SCALCE_WALK_KMER_T7 2
#define SCALCE_WALK_ANCHOR 3
int scalce_patterns_walk(const scalce_ctx *ctx, int *anchor_k);
/* core string / length by file-order index (decompress.cpp:269,341 use patterns[core]) */
int scalce_pattern_length(const scalce_ctx *ctx, int pattern);
const char *scalce_pattern_string(const scalce_ctx *ctx, int pattern);

/* Host-only description of the table builder (runs without a device): bucket_pattern_out[k] = file-order
 * index of the core whose bucket is emitted k-th (aho_output order, reads.cpp:466-499), root (0x3FFFFFFF) last. */
int scalce_patterns_describe_host(const void *blob, size_t nbytes, int is_text, int32_t *bucket_pattern_out,
                                  size_t cap, int32_t *n_states, int32_t *n_buckets);

/* scalce_patterns_walk without a device: the walk the table would select once loaded, and its anchor K.  SCALCE_WALK_NONE
 * for a table the loaders refuse. */
int scalce_patterns_walk_host(const void *blob, size_t nbytes, int is_text, int *anchor_k);

/* ---- quality model: quality_mapping_init (qualities.cpp:58-175), host only --------------- */
typedef struct {
  int32_t offset;      /* 33 or 64 */
  int32_t values[128]; /* replacement table */
} scalce_qmap;
/* stat[c] = occurrences of quality character c in the sampled records */
void scalce_qmap_init(scalce_qmap *q, const int32_t stat[128], int lossy_percentage);

/* ---- batch: one FASTQ shard resident in HBM --------------------------------------------- */
typedef struct {
  int32_t read_len[2];       /* bases per read, mate 1 / mate 2 (read_length[], compress.cpp:61) */
  int32_t paired;            /* -r */
  int32_t use_names;         /* 0 under -n */
  int32_t no_ac;             /* -A */
  scalce_qmap qmap[2];
  uint64_t bucket_set_size;  /* -B in bytes (spill rule, compress.cpp:702-715); 0 = never spill */
  /* state carried in from earlier shards of the same run (multi-GPU / multi-file); NULL = none */
  uint32_t qprev[2][2];      /* last two quality symbols before this shard, 500 = none (qualities.cpp:179) */
  /* Records without qualities (zero = FASTQ with qualities, as before).  fasta (-f): two-line records, a name line and
   * one sequence line (compress.cpp:637,662); no_qualities (-Q): four-line FASTQ whose '+' and quality lines are read and
   * dropped (compress.cpp:689,697).  Either one: no q' rows, no quality statistics, no table, no coder -- SCALCE_OUT_QUAL,
   * _TABLE, _FREQ4, _QSTREAM and _QINPUT are empty, and the -B rule counts records without quality bytes.  One GPU only:
   * scalce_sharded_compress and scalce_pipeline_create refuse such batches (SCALCE_ERR_ARG). */
  int32_t fasta;
  int32_t no_qualities;
  /* Interleaved paired-end input (-i; zero = as before).  Set together with `paired`: ONE text holds both mates, record
   * 2k + m of it is mate m of pair k.  scalce_batch_ingest takes it as mate 0 (mate 1 is an error), scalce_batch_append
   * as d_text1 (d_text2 NULL / 0) and takes whole pairs; scalce_stream_compress reads it through rd1 alone (rd2 NULL).
   * Everything behind the ingest is -r's on the same pairs: the archive is byte for byte the one of the two split texts.
   * One GPU only: scalce_sharded_compress refuses such batches (SCALCE_ERR_ARG). */
  int32_t interleaved;
  /* Reads of different lengths (--variable-length; zero = as before: a record whose length differs from read_len is an
   * error).  Set: read_len[m] is the LONGEST read of mate m, a record may hold 0 .. read_len[m] bases, and its sequence and
   * quality lines must be equally long.  The run is the fixed-length run of the same records padded to read_len -- 'N' behind a
   * read's end, whose quality symbol is 0 -- made by a pad pass in front of the ingest: SCALCE_OUT_READS, _NAMES, _QUAL, _TABLE
   * and _PERM are those of the padded text, byte for byte, and SCALCE_OUT_LENGTHS says how long each record really was.  A record
   * longer than read_len, or one whose two lines differ, is SCALCE_ERR_FORMAT from scalce_batch_ingest / _append themselves.
   * scalce_batch_append's consumed[] stays in bytes of the caller's pieces.  Not together with fasta, no_qualities or
   * interleaved (scalce_batch_create: SCALCE_ERR_ARG); one GPU only: scalce_sharded_compress, scalce_batch_rewindow,
   * scalce_batch_text_offset and scalce_pipeline_create refuse such batches (SCALCE_ERR_ARG). */
  int32_t variable_length;
} scalce_params;

void scalce_params_default(scalce_params *p);
/* Allocates every device buffer a shard of up to max_reads records / max_text bytes per mate
 * needs.  Synchronous. */
int scalce_batch_create(scalce_ctx *ctx, const scalce_params *p, uint64_t max_reads, uint64_t max_text,
                        scalce_batch **out);
void scalce_batch_destroy(scalce_batch *b);
/* Batches that share their front-stage buffers.  Rows, tokens, tie-break events and sort scratch are dead once a shard is
 * emitted -- the coder reads the reordered stream and writes the coded one -- so batches whose front stages (ingest .. emit)
 * run one after the other on ONE stream can share a single set: 15 GB instead of 35 GB of HBM per shard in flight at
 * 50 M x 100 bp.  Outputs 5, 6, 9, 10 of a batch (tokens, permutation, q' and name lengths in input order) are only valid
 * until the next batch of the workspace starts its front stages.  Destroy the batches before the workspace. */
typedef struct scalce_workspace scalce_workspace;
int scalce_workspace_create(scalce_ctx *ctx, scalce_workspace **out);
void scalce_workspace_destroy(scalce_workspace *w);
int scalce_batch_create_shared(scalce_ctx *ctx, const scalce_params *p, uint64_t max_reads, uint64_t max_text,
                               scalce_workspace *w, scalce_batch **out);

/* record reader of thread() (compress.cpp:614-666): newline index of the FASTQ text of one
 * mate, validation of the fixed read length, 2-bit packing of the bases (getval, const.cpp:47),
 * name slicing (output_name, names.cpp:48-62).  The text is not read again once the call has returned and `stream`
 * has passed it. */
int scalce_batch_ingest(scalce_batch *b, int mate, const uint8_t *d_text, uint64_t nbytes, void *stream);
/* The record reader for inputs that do not fit HBM as text (the reference reads records one by one from files of any
 * size and spills buckets to disk, compress.cpp:614-717; here the TEXT is streamed and what is derived from it stays
 * resident: 2-bit rows, q', names, tokens -- about two thirds of the text).  scalce_batch_append takes the next piece of the
 * read stream BEHIND the rows the batch already holds: as many complete records as both mates' pieces contain (the
 * mates are read in step), consumed[m] = bytes of piece m that were used -- the caller puts the rest in front of its
 * next piece; final_piece = 1 makes a leftover an error (line count not a multiple of 4, mates of different length).
 * Ingest, quality counters (prev[] runs across pieces, qualities.cpp:179) and the tie-break of the new rows against ALL
 * rows before them (bin_size is cumulative, reads.cpp:246) are done when the call returns and the text may be
 * overwritten; scalce_batch_order / _emit / _entropy then run once over everything.  d_text* 16-byte aligned, at most
 * max_text bytes each; the row arrays grow beyond max_reads when they must.  The first append after create, reset or a
 * one-piece ingest starts a new run.  Synchronises `stream`.
 * flags: SCALCE_APPEND_FINAL = the final piece; SCALCE_APPEND_NO_QUALITY leaves the trigram counters alone (the rows were
 * counted elsewhere: sharded runs); SCALCE_APPEND_NO_TOKENIZE defers the tie-break -- scalce_batch_tokenize / _begin then
 * cover every row not tokenized yet (sharded runs resolve it across ranks once all rows are in place). */
#define SCALCE_APPEND_FINAL 1
#define SCALCE_APPEND_NO_QUALITY 2
#define SCALCE_APPEND_NO_TOKENIZE 4
int scalce_batch_append(scalce_batch *b, const uint8_t *d_text1, uint64_t n1, const uint8_t *d_text2, uint64_t n2,
                        int flags, uint64_t consumed[2], void *stream);
int scalce_batch_reset(scalce_batch *b);

/* The streaming host around scalce_batch_append -- what replaces the reader half of thread() (compress.cpp:614-671) and
 * the spill files (:708-715) for inputs of any size: one reader thread per mate pulls the stream through `rd` into
 * pinned chunks of piece_bytes (0 = 1 GiB), the chunks go up with hipMemcpyAsync while the previous piece is ingested,
 * counted and tokenized, the unconsumed tail of a piece is put in front of the next one on the device; then order, emit
 * and entropy run once over the run.  On success *out holds the results (scalce_batch_output; the caller destroys it).
 * rd(user, dst, cap) returns the bytes it stored (any number up to cap), 0 at the end of the stream, < 0 on error; it is
 * called from the reader thread of its mate only.  reads_hint sizes the row arrays (0: they grow as the run comes in).
 * flags: SCALCE_STREAM_LEAN releases device buffers as stages finish (scalce_batch_set_lean); SCALCE_STREAM_DEFER_ENTROPY
 * returns behind the emit stage -- the caller runs scalce_batch_entropy_begin on a stream of its own and fetches the
 * read and name streams while the coder works.  errbuf receives the message on failure. */
#define SCALCE_STREAM_LEAN 1
#define SCALCE_STREAM_DEFER_ENTROPY 2
#define SCALCE_STREAM_KEEP_ORDER 4  /* scalce_batch_set_keep_order on the run's batch: SCALCE_OUT_PERM outlives the lean releases */
#define SCALCE_STREAM_KEEP_COMMENTS 8  /* scalce_batch_set_keep_comments on the run's batch: SCALCE_OUT_COMMENTS holds what follows the names */
#define SCALCE_STREAM_KEEP_BASES 16  /* scalce_batch_set_keep_bases on the run's batch: SCALCE_OUT_EXCEPTIONS holds what the archive does not keep of the bases */
#define SCALCE_STREAM_KEEP_PLUS 32  /* scalce_batch_set_keep_plus on the run's batch: SCALCE_OUT_PLUS holds the records' '+' lines as entries */
/* The text's digest (--digest): every chunk of every mate stream, as it has arrived on the device and before anything is put in
 * front of it or padded, gets one scalce_crc32_device launch on the stream that orders its way into the piece; the words collect
 * in a small device array, come down behind the launches without a wait of their own and are joined on the host in input order
 * (scalce_crc32_combine): stats->crc[m] = zlib's crc32 of the stats->bytes[m] bytes rd delivered for mate stream m (-i: one text,
 * crc[0]).  Without the flag nothing of it is launched or allocated and crc[] is 0. */
#define SCALCE_STREAM_DIGEST 64
typedef int64_t (*scalce_read_fn)(void *user, void *dst, uint64_t cap);
typedef struct {
  double total_s, read_wait_s, h2d_wait_s, front_s, order_s, emit_s, entropy_s;
  uint64_t rounds, reads, bytes[2];
  uint32_t crc[2];           /* SCALCE_STREAM_DIGEST */
} scalce_stream_stats;
int scalce_stream_compress(scalce_ctx *ctx, const scalce_params *p, scalce_read_fn rd1, void *user1, scalce_read_fn rd2,
                           void *user2, uint64_t piece_bytes, uint64_t reads_hint, int flags, scalce_batch **out,
                           scalce_stream_stats *stats, char *errbuf, size_t errcap);
/* lean = 1: a stage releases the device buffers that no later stage reads (q' in input order once the reordered stream
 * exists, rows and sort scratch once the records are emitted): outputs 5, 6, 9 become unavailable, runs sized for most
 * of HBM fit. */
void scalce_batch_set_lean(scalce_batch *b, int lean);
/* on = 1: the permutation is an output of the run (the order stream of --keep-order): SCALCE_OUT_PERM stays valid behind
 * scalce_batch_emit and scalce_batch_finish whether the batch is lean or not.  Nothing else changes. */
int scalce_batch_set_keep_order(scalce_batch *b, int on);
/* on = 1: what follows the name on every record's header line is an output of the run (the comment stream of --keep-comments).
 * The name slicer ends a name at the first space (output_name, names.cpp:55-57); a record's ENTRY is the rest of the line, from
 * that space inclusive to the newline exclusive -- empty for a line without a space, " " for "@name ".  Every piece's entries go,
 * each with a newline behind it, into a byte store per mate in input order (mate 2's header line has an entry of its own,
 * although its name is not stored; interleaved text: record 2k + m goes to mate m's store), and the emit stage gathers them
 * through the permutation: SCALCE_OUT_COMMENTS.  Every other output is what it is without the option, byte for byte.  An entry
 * longer than 65535 bytes is SCALCE_ERR_FORMAT from the ingest itself ("(ERROR) record <n>: what follows the name is longer than
 * 65535 bytes").  To be called before the first ingest or append of a run.  SCALCE_ERR_ARG for a batch with use_names == 0;
 * one GPU only: scalce_sharded_compress, scalce_batch_rewindow, scalce_batch_text_offset and scalce_pipeline_create refuse such
 * batches (SCALCE_ERR_ARG).  Off (the default): no kernel of it is launched and no buffer of it allocated. */
int scalce_batch_set_keep_comments(scalce_batch *b, int on);
/* *nbytes = the size of SCALCE_OUT_COMMENTS of `mate` (entries and their newlines), *longest = its longest entry in bytes without
 * the newline (the C of the .scalcec header); either may be NULL.  Valid behind the ingest of the run's last piece; zero without
 * the option. */
int scalce_batch_comments_info(const scalce_batch *b, int mate, uint64_t *nbytes, uint32_t *longest);
/* on = 1: every record's third line becomes an output of the run (the plus-line stream of --keep-plus).  It mirrors
 * scalce_batch_set_keep_comments.  The reference writes the line back as a bare '+' (decompress.cpp prints "+\n"); a record's
 * ENTRY says what stood there: empty for a bare '+'; the byte '=' when the line behind its '+' equals the header line behind
 * its '@' (the whole line, name and what follows it); else '\'' followed by the line's bytes behind the '+'.  Every piece's
 * entries go, each with a newline behind it, into a byte store per mate in input order (interleaved text: record 2k + m goes to
 * mate m's store; pieces cut anywhere), and the emit stage gathers them through the permutation: SCALCE_OUT_PLUS.  Every other
 * output is what it is without the option, byte for byte.  SCALCE_ERR_FORMAT from the ingest itself for a third line that is
 * empty or begins with another character ("(ERROR) record <n>: the third line does not begin with '+'") and for a stored entry
 * above 65535 bytes ("(ERROR) record <n>: the '+' line is longer than 65535 bytes").  To be called before the first ingest or
 * append of a run.  SCALCE_ERR_ARG for a batch made with fasta or no_qualities (no such line) or coded in place; one GPU only:
 * scalce_sharded_compress, scalce_batch_rewindow, scalce_batch_text_offset, scalce_batch_set_code_in_place and
 * scalce_pipeline_create refuse such batches (SCALCE_ERR_ARG).  Off (the default): no kernel of it is launched and no buffer of
 * it allocated. */
int scalce_batch_set_keep_plus(scalce_batch *b, int on);
/* Mirrors scalce_batch_comments_info.  *nbytes = the size of SCALCE_OUT_PLUS of `mate` (entries and their newlines), *longest =
 * its longest stored entry in bytes, class byte included, newline not (the P of the .scalcep header; 0: every line was bare),
 * *repeats / *literals = how many entries are '=' / begin with '\'' (valid behind scalce_batch_emit).  Any may be NULL. */
int scalce_batch_plus_info(const scalce_batch *b, int mate, uint64_t *nbytes, uint32_t *longest, uint64_t *repeats, uint64_t *literals);
/* on = 1: every base letter and the quality under an N become an output of the run (the exception stream of --keep-bases).  The
 * archive stores a base in two bits: a c g t as A C G T, every other letter as A (getval, const.h:127, const.cpp:47-49); an
 * upper-case N survives only by forcing quality symbol 0 (qualities.cpp:183), and every symbol 0 comes back as N
 * (decompress.cpp:350-351).  With the input's letter b and quality character q at a position, values[] / offset the run's
 * quality map: the stored symbol is s = 0 if b == 'N', else values[q] - offset (runs with qualities only); the letter that comes
 * back is 'N' if the run has qualities and s == 0, else "ACGT"[getval(b)]; the quality that comes back is offset + s.  The
 * position is an EXCEPTION when that letter is not b, or when the run has qualities, b == 'N' and values[q] != offset.  (An N with
 * the offset quality is none.)  Its ENTRY is a u64: bits 0-7 b, bits 8-15 values[q] (0 without qualities), bits 16-27 the
 * position, bits 28-63 the record's index in archive order (pairs: the pair's; each mate has its own entries).  Every piece's
 * entries go into a store per mate in input order (a count pass over the text the ingest read, a scan, a write pass), and the
 * emit stage gathers them through the permutation: SCALCE_OUT_EXCEPTIONS, strictly ascending.  Every other output is what it is
 * without the option, byte for byte.  Read lengths up to 4095.  To be called before the first ingest or append of a run
 * (SCALCE_ERR_ARG behind it); one GPU only: scalce_sharded_compress, scalce_batch_rewindow, scalce_batch_text_offset and
 * scalce_pipeline_create refuse such batches (SCALCE_ERR_ARG).  Off (the default): no kernel of it is launched and no buffer of
 * it allocated. */
int scalce_batch_set_keep_bases(scalce_batch *b, int on);
/* *entries = the u64 entries of SCALCE_OUT_EXCEPTIONS of `mate` (the X of the .scalcex header), *records_with_one = how many of
 * the mate's records hold at least one; either may be NULL.  Valid behind the ingest of the run's last piece; zero without the
 * option. */
int scalce_batch_exceptions_info(const scalce_batch *b, int mate, uint64_t *entries, uint64_t *records_with_one);
/* Row layout of the batch.  A single-end batch with names keeps ONE row per read -- q' | name cell | packed bases, what the
 * reference keeps per read in its bucket blob (reads.h:52-58, compress.cpp:675-706) -- so that the emit stage reaches
 * everything it reorders through one random access.  on = 0 (before anything is ingested) goes back to separate arrays whose
 * rows lie back to back: for callers that read SCALCE_OUT_QINPUT as one array (sharded runs); lean batches do so by themselves.
 * Returns SCALCE_ERR_ARG when the batch cannot take the layout asked for. */
int scalce_batch_set_fused_rows(scalce_batch *b, int on);
/* Where the reordered q' stream of the emit stage lives (arithmetic.cpp:318-363 cuts it into 10 MiB blocks).  on = 1: in the
 * workspace the batch shares with others instead of in the batch itself -- for callers that pass the stream on right behind
 * the emit stage and never code it where it lies (scalce_sharded_compress: every rank hands its stream to the owners of the
 * run-wide block ranges): SCALCE_OUT_QSTREAM is then valid until the next batch of the workspace runs its emit stage, and the
 * batch holds 5 GB less per 50 M reads of 100 bp.  Not with -A (the stream is the output) or lean batches: SCALCE_ERR_ARG. */
int scalce_batch_set_stream_scratch(scalce_batch *b, int on);
/* Coding in place.  on = 1: in grouped launches (scalce_batch_entropy_begin_group) the coder writes block k's bytes over block
 * k's own symbols -- the output of a block lags its input (arithmetic.cpp:85-169 emits fewer bits than it reads symbols' worth)
 * -- and the batch holds no block buffers (3.2 GB less per 50 M reads of 100 bp; SCALCE_OUT_QSTREAM is gone once the shard is
 * coded).  A block whose output would catch up with its input cannot be coded again from symbols that are already
 * overwritten: the shard is then run again from its TEXT with buffers of its own when it is collected, so the caller keeps
 * the text passed to scalce_batch_front / _ingest where it is until the shard has been collected.  Not with -A or lean
 * batches (SCALCE_ERR_ARG); a stream handed in by the caller (sharded runs) is never coded in place. */
int scalce_batch_set_code_in_place(scalce_batch *b, int on);
uint64_t scalce_batch_reruns(const scalce_batch *b);  /* shards of this batch that had to be run again from their text */
int scalce_batch_coder_round(const scalce_batch *b);  /* symbols per round of the last one-block-per-lane coder launch this batch led; 0: none */
/* For tests: the path the last scalce_batch_quality call took for `mate`.  out = {source, lo, A, inside}: source = where the
 * symbol range came from -- 0: nothing was counted (-A, no qualities, an empty piece), 1: the tile ranges the one-pass ingest
 * left, 2: a scan of the piece's q' rows, 3: the whole alphabet (fused rows without tile ranges); lo, A = first symbol and
 * span of the counters laid out, inside = 1 when no symbol of the piece lies outside them (all 0 when source is 0).
 * Waits for the whole device and reads the three back. */
int scalce_batch_quality_plan(const scalce_batch *b, int mate, uint32_t out[4]);
/* For tests: what the ingest of the last piece (scalce_batch_ingest, _append, _front, _compress) did for `mate`.
 * out[0] = the kernel that wrote the mate's rows -- 0: nothing ingested yet, or an empty piece, 1: the one-pass tile kernel
 * (read lengths 16 .. 160), 2: the indexed kernel that works out of LDS tiles (read lengths up to 160), 3: the indexed kernel
 * that reads every record straight from memory (longer reads); out[1] = 1 when the one-pass kernel ran first, met a record that
 * does not end inside its tile's overlap (or a tile with more than 2048 lines) and the piece was done again by an indexed
 * kernel; out[2] = 1 when the line index of the piece was built on the way (the indexed kernels and names longer than 15
 * characters need it); out[3] = the bytes the piece added to the store of names longer than 15 characters (mate 0; 0 for
 * mate 1 of two texts).  Interleaved batches ingest both mates from one text: mate 1 reports mate 0's out[1..3], and in out[0]
 * the kernel that wrote its own rows.  Host bookkeeping only: nothing is launched, waited for or read back. */
int scalce_batch_ingest_plan(const scalce_batch *b, int mate, uint32_t out[4]);
/* edge[0..1] = the first two, edge[2..3] = the last two q' symbols of the rows held (input order), *nsym = how many there are,
 * *read_len (may be NULL) = symbols per row: what a rank of a sharded run tells its neighbours (qualities.cpp:179-198: prev[]
 * runs across reads, so two trigrams straddle every rank boundary).  Runs on `stream` and synchronises it. */
int scalce_batch_qinput_edges(scalce_batch *b, int mate, uint8_t edge[4], uint64_t *nsym, int32_t *read_len, void *stream);
/* output_quality (qualities.cpp:177-204): q' = map[q]-offset (N -> 0) and the order-2 trigram
 * counters ac_freq4 over the input-order stream of this shard. */
int scalce_batch_quality(scalce_batch *b, void *stream);
/* aho_search (reads.cpp:413-429) for every read, including the cumulative bin_size tie-break
 * resolved exactly in input order (-T 1 semantics).  d_prior_counts: per-bucket counts of reads
 * assigned by EARLIER shards (bucket order = scalce_bucket_*), or NULL. */
int scalce_batch_tokenize(scalce_batch *b, const uint64_t *d_prior_counts, void *stream);
/* The same in two halves: _begin (both walks, candidates, events, first counts) and _settle (below).  A run sharded over
 * several GPUs calls _begin on every rank at once and _settle rank by rank: rank r settles against the counts of ranks
 * 0 .. r-1 (d_prior_counts = their sum per bucket), then hands its own SCALCE_OUT_BUCKET_COUNTS on (scalce_sharded_compress). */
int scalce_batch_tokenize_begin(scalce_batch *b, void *stream);
int scalce_batch_tokenize_end(scalce_batch *b, void *stream);
/* scalce_batch_tokenize = _begin + _settle: _settle resolves the tie-break of this batch on its own against fixed prior
 * counts (window by window in input order) and ends the tokenization.  Split so that a caller can enqueue other work of the
 * shard on a second stream beside the tie-break's many small launches. */
int scalce_batch_tokenize_settle(scalce_batch *b, const uint64_t *d_prior_counts, void *stream);
/* Sharded runs: the cuts the -B rule makes inside this batch's rows when `carry_in` bytes of records are already in the
 * chunk that is open where they begin (the rows of the ranks before): cuts_host[i] = row in front of which chunk i + 1
 * begins (1 .. N; at most cap), carry_out = bytes in the chunk still open behind the last row.  Needs the rows ingested,
 * not tokenized (record sizes depend on the core's length only).  *ncuts == cap says that the list may be cut short: the
 * cuts returned are the first cap of the plan, *carry_out is then the size of every row behind the last of them and no
 * carry.  A caller passes a cap above any plan it accepts and takes *ncuts == cap for SCALCE_ERR_CAPACITY
 * (scalce_sharded_compress: SCALCE_SHARD_CUT_CAP cuts per rank).  A batch without rows: no cuts, *carry_out = carry_in. */
#define SCALCE_SHARD_CUT_CAP 4000
int scalce_batch_chunk_plan(scalce_batch *b, uint64_t carry_in, uint64_t *cuts_host, uint32_t cap, uint32_t *ncuts,
                            uint64_t *carry_out, void *stream);
/* Byte offset, in the text of the piece ingested last, at which record `row` (0 .. rows of that piece) begins; runs on
 * `stream`, behind the ingest of that piece. */
int scalce_batch_text_offset(scalce_batch *b, int mate, uint64_t row, uint64_t *offset, void *stream);
/* Sharded runs: the row range a rank holds changes at both ends once the run-wide spill-chunk cuts are known (rank boundaries
 * move to the nearest cut, compress.cpp:702-715): rows [keep_first, keep_first + keep_rows) of the batch stay as they are, the
 * records of `front` (FASTQ text on the device, whole records, 16-byte aligned; [mate]) become rows in front of them, those of
 * `back` rows behind them.  Only the records that arrive are ingested and walked; the quality statistics are not touched (every
 * record was counted by the rank that ingested it first).  Before any tokenization of the batch (SCALCE_ERR_ARG behind one, and
 * for an interleaved batch, nothing has moved then); a text that does not end with its last record, or whose mates hold different
 * numbers of records, is SCALCE_ERR_FORMAT ("rewindow: the front / back text is not whole records: ..."): the batch has given up
 * its rows by then, and scalce_batch_reset or a new ingest starts it over. */
int scalce_batch_rewindow(scalce_batch *b, uint64_t keep_first, uint64_t keep_rows, const uint8_t *const front[2],
                          const uint64_t front_bytes[2], const uint8_t *const back[2], const uint64_t back_bytes[2], void *stream);
/* Spill-chunk boundaries given by the caller instead of the -B rule: starts[0] = 0 < starts[1] < ...;
 * records of chunk i precede those of chunk i+1 inside every bucket (merge order, compress.cpp:104-159).
 * A sharded run uses one chunk per shard. */
int scalce_batch_set_chunks(scalce_batch *b, const uint64_t *starts, uint32_t n);
/* aho_trie_bucket + aho_output + bin_prepare/_radix_sort (reads.cpp:233-250,466-499,547-634)
 * + the merge order of spilled chunks (compress.cpp:104-159): the output permutation. */
int scalce_batch_order(scalce_batch *b, void *stream);
/* output_read (reads.cpp:432-461) + bin_dump (:91-180) + per-bucket headers
 * (compress.cpp:364-379): the .scalcer / .scalcen payloads and the reordered quality stream. */
int scalce_batch_emit(scalce_batch *b, void *stream);
/* table scaling (compress.cpp:296-320), ac_stat (arithmetic.cpp:54-78) and ac_write /
 * ac_coder (:85-169,318-363): [u32 size][bytes] per 10 MiB block of the reordered stream.
 * d_table_override (512000 x u32 per mate, already scaled) replaces this shard's own
 * statistics when the run-wide table was reduced across shards; NULL = use own. */
int scalce_batch_entropy(scalce_batch *b, const uint32_t *d_table_override, void *stream);
/* The same stage in two halves, for callers that keep several shards in flight: _begin only enqueues (table,
 * coder, framing -- one short wait for the table's largest context total, none for the coder), so the caller
 * can run the front stages of the next shard on another stream while the coder -- a long kernel that leaves
 * most of the chip idle, one wavefront per 10 MiB block -- works in the background; _end (or
 * scalce_batch_finish) waits for it and fills in the size of SCALCE_OUT_QUAL.  This is the device-side
 * counterpart of the reference coding `-T` blocks per batch on its thread pool (arithmetic.cpp:349-357). */
int scalce_batch_entropy_begin(scalce_batch *b, const uint32_t *d_table_override, void *stream);
int scalce_batch_entropy_end(scalce_batch *b, void *stream);
/* The begin half for several shards at once: ONE coder launch over the blocks of all of them, with several blocks per
 * chain wavefront (four: 0.57 x the SIMD time per block of the one-block kernel at 1.13 x its latency; eight: ~0.35 x
 * at 1.3 x).  The library picks the fewest blocks per wave that keep the launch at one workgroup per CU -- two
 * 50 M-read shards are 954 blocks = 239 workgroups of four, three shards 179 workgroups of eight -- so every coder wave
 * has a SIMD to itself by construction and the group is coded in little more than the time one shard takes.  Tables
 * are prepared on prep_stream (the host waits there, never behind a running coder), the coder and the framing are
 * enqueued on stream.  Each shard is completed by its own scalce_batch_entropy_end / scalce_batch_finish (on any
 * stream, after `stream` has reached the end of the launch). */
int scalce_batch_entropy_begin_group(scalce_batch **batches, int n, void *prep_stream, void *stream);
#define SCALCE_GROUP_MAX 16  /* shards per grouped launch (n), and so the largest `group` of scalce_pipeline_create */
/* The same for the LAST launch of a run (last == 1: nothing will be queued behind it): picks the coder kernel by how soon
 * the launch is done instead of by how few CUs it holds beside the next shards' front stages.  last == 0 is
 * scalce_batch_entropy_begin_group; any other value is SCALCE_ERR_ARG.  Same bytes. */
int scalce_batch_entropy_begin_group_last(scalce_batch **batches, int n, void *prep_stream, void *stream, int last);
/* Sharded runs: code a caller-assembled range of the run-wide reordered stream (it must start on a 10 MiB
 * block boundary) against the run-wide table; result in SCALCE_OUT_QUAL of `mate`. */
int scalce_batch_entropy_stream(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                uint64_t nsym, void *stream);
int scalce_batch_entropy_stream_begin(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                      uint64_t nsym, void *stream);
/* ... or only remembered, to be coded by the next scalce_batch_entropy_begin_group that includes this shard. */
int scalce_batch_entropy_stream_prepare(scalce_batch *b, int mate, const uint32_t *d_table, const uint8_t *d_symbols,
                                        uint64_t nsym, void *stream);
/* Table scaling on its own (compress.cpp:297-313): d_table[i] = max(1, (1 + d_counters[i]) / factor) for the 512000
 * counters of one mate (SCALCE_OUT_FREQ4 layout: raw trigram counts; the reference's counters all start at 1,
 * qualities.cpp:191-196).  factor = 1 + symbols / (2^32 - 1) over the RUN (:297-303). */
int scalce_ac_scale(scalce_ctx *ctx, const uint64_t *d_counters, uint32_t factor, uint32_t *d_table, void *stream);
/* Piecewise device copy: dst[piece_dst[p] + i] = src[piece_src[p] + i]; pieces contiguous in src, sorted. */
int scalce_copy_pieces(scalce_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, const uint64_t *d_piece_src,
                       const uint64_t *d_piece_dst, uint32_t npieces, uint64_t total_bytes, void *stream);
/* all of the above in order */
int scalce_batch_compress(scalce_batch *b, const uint8_t *d_text1, uint64_t n1, const uint8_t *d_text2,
                          uint64_t n2, void *stream);
/* Every stage in front of the entropy coder (ingest .. emit) of a shard resident as text (mate 2: NULL / 0 for single-end). */
int scalce_batch_front(scalce_batch *b, const uint8_t *d_text1, uint64_t n1, const uint8_t *d_text2, uint64_t n2, void *stream);
/* Synchronises `stream`, checks the device error word, fills the host-side result sizes. */
int scalce_batch_finish(scalce_batch *b, void *stream);

/* results (device pointers owned by the batch; sizes valid after scalce_batch_finish) */
enum {
  SCALCE_OUT_READS = 0,     /* .scalcer payload after the 16-byte header, mate m            */
  SCALCE_OUT_NAMES = 1,     /* .scalcen payload after magic+flag (empty under -n), mate 1    */
  SCALCE_OUT_QUAL = 2,      /* .scalceq payload after header+table+total: AC blocks, or raw q' under -A */
  SCALCE_OUT_TABLE = 3,     /* 512000 x u32 scaled frequency table (file order), mate m      */
  SCALCE_OUT_FREQ4 = 4,     /* 512000 x u64 raw trigram counters of this shard, mate m       */
  SCALCE_OUT_TOKENS = 5,    /* N x {int32 pattern (file order, -1 = none), int32 end}, input order */
  SCALCE_OUT_PERM = 6,      /* N x u32: input index of the k-th emitted record               */
  SCALCE_OUT_QSTREAM = 7,   /* N*L bytes: reordered q' stream, mate m                         */
  SCALCE_OUT_BUCKET_COUNTS = 8, /* (buckets+1) x u64 reads per bucket, emission order, root last */
  SCALCE_OUT_QINPUT = 9,    /* N*L bytes: q' in input order, mate m                          */
  SCALCE_OUT_NAMELEN = 10,  /* N bytes: stored name length per read, input order             */
  SCALCE_OUT_BUCKET_NAME_BYTES = 11, /* (buckets+1) x u64: bytes of each bucket's records in SCALCE_OUT_NAMES (after emit) */
  SCALCE_OUT_LENGTHS = 12,  /* variable-length runs: N x u16, read_len - length of the k-th emitted record of mate m (mate 2 in
                               mate 1's order, like its reads); valid behind scalce_batch_order; empty for other runs */
  SCALCE_OUT_NAMECELLS = 13,/* for tests: N x 16 bytes, input order: [stored length][the name's first 15 characters, zero behind a
                               shorter name] as the ingest left them; empty with names off, gone once a lean batch has emitted */
  SCALCE_OUT_COMMENTS = 14, /* scalce_batch_set_keep_comments: what follows the name of the k-th emitted record of mate m, each entry
                               followed by a newline (mate 2 in mate 1's order); valid behind scalce_batch_emit, lean or not; empty
                               without the option */
  SCALCE_OUT_EXCEPTIONS = 15,/* scalce_batch_set_keep_bases: the u64 entries of mate m in archive order, strictly ascending (letter |
                               values[q] << 8 | position << 16 | record << 28); valid behind scalce_batch_emit, lean or not; empty
                               without the option */
  SCALCE_OUT_PLUS = 16       /* scalce_batch_set_keep_plus: the '+'-line entry of the k-th emitted record of mate m, each followed by a
                                newline (mate 2 in mate 1's order); valid behind scalce_batch_emit, lean or not; empty without the option */
};
int scalce_batch_output(const scalce_batch *b, int which, int mate, const void **d_ptr, uint64_t *nbytes);
/* Framing on the way out (replaces the copy loop of ac_write, arithmetic.cpp:318-363: the reference frames each coded
 * block -- [u32 size][bytes] -- as it writes it to the file).  With frame_on_demand set, the entropy stage leaves the coded
 * blocks where the coder wrote them and only lays the frames out; scalce_batch_qual_window then delivers bytes
 * [offset, offset + nbytes) of SCALCE_OUT_QUAL into dst -- device memory, or pinned host memory (4-byte aligned): the
 * framing kernel's stores are the download -- so the stream never exists a second time in HBM.  Valid after
 * scalce_batch_finish / _entropy_end.  A caller that asks scalce_batch_output for SCALCE_OUT_QUAL still gets the whole
 * stream as one device buffer; it is put together at that moment. */
int scalce_batch_set_frame_on_demand(scalce_batch *b, int on);
int scalce_batch_qual_bytes(const scalce_batch *b, int mate, uint64_t *nbytes);  /* size of SCALCE_OUT_QUAL, nothing put together */
int scalce_batch_qual_window(scalce_batch *b, int mate, uint64_t offset, uint64_t nbytes, void *dst, void *stream);
uint64_t scalce_batch_reads(const scalce_batch *b);
int scalce_batch_params(const scalce_batch *b, scalce_params *out);  /* the parameters it was created with */
/* measurement hook for bench.py: accumulated device time (ms, hipEvent) and launch count of
 * stage `which` (0 ingest,1 quality,2 tokenize,3 order,4 emit,5 entropy) since the last reset */
int scalce_batch_stage_ms(scalce_batch *b, int which, float *ms, int *launches);
void scalce_batch_stage_reset(scalce_batch *b, int enable);

/* HIP-event pairs around every launch of the dominant kernel (ac_encode_k) on the caller's stream.
 * kernel_timing(1) arms and clears; kernel_ms synchronises the recorded events and returns the summed
 * duration, the launch count and the algorithmic bytes (symbols read, coded bytes written). */
void scalce_batch_kernel_timing(scalce_batch *b, int enable);
int scalce_batch_kernel_ms(scalce_batch *b, double *total_ms, int *launches, uint64_t *bytes_in, uint64_t *bytes_out);

/* plumbing for hosts without a HIP binding of their own (ctypes, cgo): blocking copies */
int scalce_memcpy_d2h(scalce_ctx *ctx, void *dst_host, const void *src_dev, uint64_t nbytes);
int scalce_memcpy_h2d(scalce_ctx *ctx, void *dst_dev, const void *src_host, uint64_t nbytes);
int scalce_memcpy_d2d(scalce_ctx *ctx, void *dst_dev, const void *src_dev, uint64_t nbytes, void *stream); /* async */
/* diagnostics of the last run: tie reads, candidate events, fixed-point sweeps, spill chunks, records that
 * needed the second sort phase, 1 if the tie-break ended in the sequential fallback (tie_sequential_k), the second
 * sort phase's `any_large` as read back: != 0 when a run of more than 32 records with bases behind the 16-base prefix sent
 * every run through the radix passes, 0 when the runs were sorted where they stood or the phase did not run */
int scalce_batch_stats(const scalce_batch *b, uint32_t out[7]);
/* For tests: the path the last tie-break (scalce_batch_tokenize, _tokenize_settle) took.  out[0] = 0: the piece had no tie
 * reads, 1: windows of tie reads with one launch per sweep, 2: windows with two launches per sweep (a window whose words do
 * not fit a workgroup's LDS, or SCALCE_TIE_WINDOW=<reads>:two_launches), 3: the global sweeps (SCALCE_TIE_WINDOW=0); out[1] =
 * the tie reads per window actually used, after the clamp to 2^30 and the cap of 64 Mi cells (windows x (buckets + 1)),
 * out[2] = the number of windows (both 0 without windows); out[3] = where tie_sequential_k kept its counters when the sweeps
 * gave up (scalce_batch_stats out[5]) -- 1: LDS inside the default limit (up to 48 KB of counters), 2: LDS with the limit raised (up to 100 KB), 3: global memory,
 * 0: it did not run.
 * Host bookkeeping only: nothing is launched, waited for or read back. */
int scalce_batch_tie_plan(const scalce_batch *b, uint32_t out[4]);

/* Device self-test of the arithmetic coder's closed-form step (multiply-high by reciprocal fractions, merged
 * renormalisation shift) against the literal loop of arithmetic.cpp:122-152 on `ncases` random and crafted
 * states.  general = 0: the production step on well-formed states with totals <= 2^30; general = 1: the
 * all-states step, including inverted intervals; general = 2: the plain-round step on the (lo, range) state with
 * its fall-back, as the encoder's inner loop runs it.  out[0] = mismatches, out[1..5] = lo, hi, c_lo, c_hi, total of the first one. */
int scalce_selftest_ac(scalce_ctx *ctx, uint64_t ncases, uint32_t seed, int general, uint32_t out[6]);

/* ---- zlib's CRC-32 of a text on the device (kernels_crc.hpp; --digest and the check on -d) -----------------------------
 * Polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF: the number gzip keeps in a member's trailer.
 * scalce_crc32_device enqueues two launches on `stream` (spans of the range, each by one workgroup; then the join of the
 * workgroups' words) and nothing else: behind them *d_crc holds crc32(0, data, nbytes).  d_data: any byte address, nothing
 * outside [d_data, d_data + nbytes) is read; nbytes 0 .. 2^40 (0: *d_crc = 0).  ws: device scratch of
 * scalce_crc32_ws_bytes(nbytes) bytes, 4-byte aligned, the launch's own until it has run.
 * scalce_crc32_plan (no device call) says how a range that begins on a 16-byte boundary is cut: out = {bytes per lane per
 * step, bytes per workgroup step (tile), bytes per workgroup (span: whole tiles), workgroups launched}.  A range that begins
 * h bytes behind such a boundary is cut like one of h + nbytes bytes.
 * scalce_crc32_combine (host only): crc32(A || B) from crc32(A), crc32(B) and B's length -- zlib's crc32_combine64 --, what
 * joins the results of chunks, windows and stripes in order. */
int scalce_crc32_device(scalce_ctx *ctx, const uint8_t *d_data, uint64_t nbytes, uint32_t *d_crc, void *ws, void *stream);
uint64_t scalce_crc32_ws_bytes(uint64_t nbytes);
int scalce_crc32_plan(uint64_t nbytes, uint32_t out[4]);
uint32_t scalce_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- decode side (next row of SURVEY 8f-1): ac_read / ac_decoder (arithmetic.cpp:173-268,
 *      365-400).  d_blocks = [u32 size][bytes]... as written by scalce_batch_entropy. ---------- */
int scalce_ac_decode(scalce_ctx *ctx, const uint32_t *table_host, const uint8_t *d_blocks, uint64_t nbytes,
                     uint64_t nsymbols, uint8_t *d_symbols_out, void *stream);

/* The same decoder in two steps, for a caller that decodes a stream in runs of whole frames (scalce_stream_decompress):
 * scalce_ac_decoder_create prepares once per archive what depends on the table alone -- interval table, compact rows, the
 * ranking of the hot symbols, the choice of kernel --; scalce_ac_decoder_launch enqueues the decode of `nframes` whole
 * frames that begin at d_frames (any frame of the stream) into d_symbols_out: nsymbols of them, SCALCE_AC_BLOCK per frame
 * but the last of the stream.  d_off / d_size (nframes entries each) and d_bad (one word) are device scratch of the
 * caller: the frame walk fills them on the stream, the decoder reads them; *d_bad != 0 afterwards: the bytes end before
 * the frames do ("(ERROR) truncated quality stream").  The launch allocates nothing and waits for nothing. */
typedef struct scalce_ac_decoder scalce_ac_decoder;
int scalce_ac_decoder_create(scalce_ctx *ctx, const uint32_t *table_host, void *stream, scalce_ac_decoder **out);
void scalce_ac_decoder_destroy(scalce_ac_decoder *d);
uint64_t scalce_ac_decoder_device_bytes(const scalce_ac_decoder *d);  /* device memory the decoder holds */
int scalce_ac_decoder_launch(scalce_ac_decoder *d, const uint8_t *d_frames, uint64_t nbytes, uint32_t nframes,
                             uint64_t nsymbols, uint64_t *d_off, uint32_t *d_size, uint32_t *d_bad, uint8_t *d_symbols_out,
                             void *stream);

/* Records back to FASTQ text on the device: the per-record body of decompress.cpp:240-366 -- bucket directory
 * (:262-270), un-rotation of the 2-bit bases around the core (:331-345), N where the quality is 0 (:350-351), name
 * line (:290-299; library mode "@<library>.<index>" :300-304), '+' line, qualities + phred offset.
 *   reads_host   .scalcer payload behind its header (magic, no_ac, read length), host memory: the directory walk
 *                is serial; has_buckets = 1 for mate 1 (bucket headers, end metadata), 0 for mate 2 (bare records,
 *                no core -- the reference's stale `corlen` of decompress.cpp:250,332 is NOT reproduced);
 *   d_qual       nrecords * read_len quality symbols in archive order (scalce_ac_decode's output, or the raw
 *                bytes of a -A archive), device memory; NULL: two-line records (scalce_fasta_text_bytes);
 *   names_host   .scalcen payload behind magic and use_names byte, or NULL for library mode (`library` used);
 *   mate_digit   0, or '1' / '2' for paired archives: a name ending in "/x" gets this digit (:296-298);
 *   d_out        device buffer of out_cap >= scalce_fastq_text_bytes(...) bytes;
 *   record_offsets_host  optional, nrecords + 1 entries: where each record starts in the text (-S splitting).
 * Returns when the text is complete. */
uint64_t scalce_fastq_text_bytes(int read_len, uint64_t nrecords, uint64_t names_bytes, const char *library /* NULL: names */);
/* The same for the two-line records of an archive without qualities (-Q / -f): "@name\n" + bases + "\n" per record
 * (decompress.cpp:323-366 with _compress_qualities = 0).  scalce_fastq_records writes them when d_qual is NULL: no '+'
 * line, no quality line, no N restore (a base stored as 0 comes back as 'A'). */
uint64_t scalce_fasta_text_bytes(int read_len, uint64_t nrecords, uint64_t names_bytes, const char *library /* NULL: names */);
int scalce_fastq_records(scalce_ctx *ctx, int read_len, int has_buckets, const uint8_t *reads_host, uint64_t reads_bytes,
                         uint64_t nrecords, const uint8_t *d_qual, int64_t phred_offset, const uint8_t *names_host,
                         uint64_t names_bytes, const char *library, int mate_digit, uint8_t *d_out, uint64_t out_cap,
                         uint64_t *out_bytes, uint64_t *record_offsets_host, void *stream);
/* Both mates of a paired archive into ONE interleaved text (-d -i): mate 1 of pair k, then mate 2 of pair k.  Arguments are
 * scalce_fastq_records' per mate ([0]: mate 1, whose read stream has the bucket headers; [1]: mate 2); each record's bytes
 * are the ones scalce_fastq_records writes for it with mate_digit '1' / '2'.  Both mates hold `npairs` records.
 * out_bytes = the sum of both mates' text sizes; pair_offsets_host (optional, npairs + 1 entries): where each pair starts. */
int scalce_fastq_records_interleaved(scalce_ctx *ctx, const int read_len[2], const uint8_t *const reads_host[2],
                                     const uint64_t reads_bytes[2], uint64_t npairs, const uint8_t *const d_qual[2],
                                     const int64_t phred_offset[2], const uint8_t *const names_host[2],
                                     const uint64_t names_bytes[2], const char *library, uint8_t *d_out, uint64_t out_cap,
                                     uint64_t *out_bytes, uint64_t *pair_offsets_host, void *stream);

/* One WINDOW of whole records of an archive, everything on the device and relative to the window: what
 * scalce_fastq_records does for a whole archive, enqueued for records first_record .. first_record + nrecords - 1.
 *   d_reads      the slice of the read stream from the window's first record on; bucket headers stay inline;
 *   d_dir        the buckets that have records in the window: `first` counts from the window's first record, `off` from
 *                d_reads (has_buckets = 0, mate 2: one entry, core_len 0, rec_bytes = (read_len + 3) / 4);
 *   d_qual       the window's first symbol, any byte address; NULL: two-line records;
 *   d_names / d_name_off   the window's name records and where each starts in them (nrecords + 1 entries), or NULL / NULL:
 *                library mode, names "<library>.<first_record + k>";
 *   d_out        the window's text;  d_record_offsets (optional, nrecords + 1): where each record starts in it;
 *   interleave   0, or 1 / 2 for mate 1 / 2 of an interleaved text: both mates of the window go into ONE window text,
 *                pair_read_len and d_pair_name_off (the other mate's, nrecords + 1 entries) say where. */
typedef struct {
  uint64_t first, off;     /* first record of the bucket (window-relative), byte offset of that record in d_reads */
  uint32_t core_len, rec_bytes;
  char core[32];
} scalce_fq_bucket;
typedef struct {
  const uint8_t *d_reads;
  const scalce_fq_bucket *d_dir;
  uint32_t nbuckets;
  int32_t read_len, has_buckets, mate_digit;
  uint64_t nrecords, first_record;
  const uint8_t *d_qual;
  int64_t phred_offset;
  const uint8_t *d_names;
  const uint64_t *d_name_off;
  const char *library;
  uint8_t *d_out;
  uint64_t *d_record_offsets;
  int32_t interleave, pair_read_len;
  const uint64_t *d_pair_name_off;
} scalce_fq_window;
int scalce_fastq_records_window(scalce_ctx *ctx, const scalce_fq_window *w, void *stream);

/* Variable-length archives: the pad behind each read's end is cut out of a window's text.  d_text / d_record_offsets are what
 * scalce_fastq_records_window wrote (one mate's four-line records, not interleaved; nrecords + 1 offsets), d_entries the
 * window's entries of the length stream as the .scalcel file holds them: entry_width (1 or 2) bytes each, little-endian,
 * read_len - length.  The record's last `entry` bases and qualities go; d_out receives the text, d_out_offsets (nrecords + 1)
 * where each record begins in it and, last, its size.  d_text and d_out 16-byte aligned; d_scan_ws: device scratch of
 * scalce_fastq_strip_ws_bytes(nrecords) bytes.  Enqueued on `stream`; allocates nothing, waits for nothing. */
uint64_t scalce_fastq_strip_ws_bytes(uint64_t nrecords);
int scalce_fastq_strip_window(scalce_ctx *ctx, int read_len, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets,
                              const uint8_t *d_entries, int entry_width, uint8_t *d_out, uint64_t *d_out_offsets, void *d_scan_ws,
                              void *stream);

/* Archives made with --keep-comments: the entries of the comment stream go back between each name and its newline.  d_text /
 * d_record_offsets are what scalce_fastq_records_window wrote (one mate's records, not interleaved; nrecords + 1 offsets; records
 * of read_len bases, has_qualities = 0 for two-line records: the header line's newline lies 2 read_len + 5, or read_len + 2,
 * bytes in front of the record's end), d_entries the window's entry_bytes bytes of the stream as the .scalcec file holds them
 * behind its header: nrecords entries, each followed by a newline.  Where each entry lies is found on the device by a newline
 * index.  d_out receives the text (room for the window's text plus entry_bytes), d_out_offsets (nrecords + 1) where each record
 * begins in it and, last, its size.  *d_bad is set when the entries do not hold exactly nrecords newlines, the last one at their
 * end (records whose entry is missing then get none).  To be run BEFORE scalce_fastq_strip_window, which measures from the
 * record's end.  d_text, d_entries and d_out 16-byte aligned; d_ws: device scratch of scalce_fastq_comment_ws_bytes(nrecords,
 * entry_bytes) bytes.  Enqueued on `stream`; allocates nothing, waits for nothing. */
uint64_t scalce_fastq_comment_ws_bytes(uint64_t nrecords, uint64_t entry_bytes);
int scalce_fastq_comment_window(scalce_ctx *ctx, int read_len, int has_qualities, uint64_t nrecords, const uint8_t *d_text,
                                const uint64_t *d_record_offsets, const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out,
                                uint64_t *d_out_offsets, uint32_t *d_bad, void *d_ws, void *stream);
/* The same for an interleaved window (scalce_fastq_records_window with interleave): npairs pairs, mate 1 then mate 2 of each, of
 * read_len[0] / read_len[1] bases; d_pair_offsets (npairs + 1) where each pair begins, d_name_off2 mate 2's name offsets as
 * scalce_fastq_records_window took them (npairs + 1: a name record is a length byte and the name, which is how long mate 2's
 * header line is); d_entries: 2 npairs entries, mate 1's then mate 2's of each pair.  d_out_pair_offsets (npairs + 1): where each
 * pair begins in d_out.  d_ws: scalce_fastq_comment_pairs_ws_bytes(npairs, entry_bytes) bytes. */
uint64_t scalce_fastq_comment_pairs_ws_bytes(uint64_t npairs, uint64_t entry_bytes);
int scalce_fastq_comment_window_pairs(scalce_ctx *ctx, const int read_len[2], int has_qualities, uint64_t npairs, const uint8_t *d_text,
                                      const uint64_t *d_pair_offsets, const uint64_t *d_name_off2, const uint8_t *d_entries,
                                      uint64_t entry_bytes, uint8_t *d_out, uint64_t *d_out_pair_offsets, uint32_t *d_bad, void *d_ws,
                                      void *stream);

/* Archives made with --keep-bases: the entries of the exception stream go back into a window's text, in place (what
 * decompress.cpp:331-351 cannot give back: lower case, IUPAC letters, the quality under an N, the base under symbol 0).  d_text /
 * d_record_offsets are what scalce_fastq_records_window wrote (one mate's records; nrecords + 1 offsets; records of read_len
 * bases, has_qualities = 0 for two-line records), the window holds the archive's records [first_record, first_record + nrecords),
 * d_entries the nentries u64 entries of those records as the .scalcex file holds them (device memory).  One thread per entry
 * writes the letter into the sequence line and, with qualities, the quality character into the quality line; both lines are found
 * from the record's end, so names of any length need nothing.  *d_bad is cleared, then set by an entry whose record lies outside
 * the window or whose position is not below read_len: such an entry stores nothing.  To be run BEFORE the comments go back, the
 * pad goes and the order is restored (all three keep the lines' contents).  Enqueued on `stream`; allocates nothing, waits for
 * nothing. */
int scalce_fastq_exception_window(scalce_ctx *ctx, int read_len, int has_qualities, uint64_t first_record, uint64_t nrecords,
                                  uint8_t *d_text, const uint64_t *d_record_offsets, const uint64_t *d_entries, uint64_t nentries,
                                  uint32_t *d_bad, void *stream);
/* The same for an interleaved window: npairs pairs from pair first_pair on, mate 1 then mate 2 of each, of read_len[0] /
 * read_len[1] bases; d_pair_offsets (npairs + 1), d_name_off2 mate 2's name offsets as scalce_fastq_records_window took them, or
 * NULL for made-up names ("<library>.<index>": library_len = the library name's length, else ignored);
 * d_entries[m] / nentries[m]: mate m's entries (their record index counts pairs).  d_ws: device scratch of
 * scalce_fastq_exception_pairs_ws_bytes(npairs) bytes. */
uint64_t scalce_fastq_exception_pairs_ws_bytes(uint64_t npairs);
int scalce_fastq_exception_window_pairs(scalce_ctx *ctx, const int read_len[2], int has_qualities, uint64_t first_pair, uint64_t npairs,
                                        uint8_t *d_text, const uint64_t *d_pair_offsets, const uint64_t *d_name_off2, uint64_t library_len,
                                        const uint64_t *const d_entries[2], const uint64_t nentries[2], uint32_t *d_bad, void *d_ws,
                                        void *stream);

/* The read length of a variable-length run and its quality histogram, from the text read ahead for the quality sample -- no
 * device call.  The first `sample` records r with r % stride == first are taken (sample_stats' walk; stride 1, first 0 for
 * a text of one mate): *read_len = the longest sequence line among them, or max_length when that is > 0 (--max-length);
 * stat (may be NULL; the caller clears it) counts the characters of their quality lines -- real ones only, there is no pad
 * yet.  Returns the records sampled. */
int64_t scalce_varlen_sample(const uint8_t *text, uint64_t nbytes, int64_t sample, int stride, int first, int max_length,
                             int32_t stat[128], int32_t *read_len);

/* ---- archives of any size back to text: windows of whole records through the device (stream_decode.cpp) ---------------
 * The counterpart of scalce_stream_compress.  rd[m][0..2] deliver the bytes of mate m's .scalcer, .scalcen and .scalceq
 * files, out of their containers, headers included (scalce_read_fn's contract: any number of bytes up to cap, 0 at the
 * end, < 0 on error); the library parses the headers.  The archive moves through the device in windows of whole records
 * of at most window_text_bytes of FASTQ text (at least one record; two-line records count as their four-line FASTQ): device and pinned host memory are sized from the window,
 * the read length and the core table, never from the archive.  While a window is decoded and turned into text the next
 * one is read and comes up and the previous one goes down and is handed to wr, in order, from a thread of its own:
 *   wr(user, mate, first_record, nrecords, text, nbytes, record_offsets)   text: pinned host memory, valid during the call;
 *      record_offsets (nrecords + 1 entries, window-relative) only when `split` is set, else NULL; != 0 ends the session.
 * Two mates that are not interleaved go one after the other through the same buffers (mate = 0, then 1); interleaved,
 * both mates of a window form one text (mate = 0, records = pairs).  Nothing further is launched after an error. */
typedef int64_t (*scalce_skip_fn)(void *user, uint64_t nbytes);  /* (scalce_unpack_range below says what it does) */
typedef struct {
  int32_t mates;             /* 1, or 2 (-r, -i) */
  int32_t interleave;        /* both mates into ONE text, mate 1 then mate 2 of each pair */
  int32_t no_qualities;      /* two-line records; the .scalceq streams are not read (rd[m][2] may be NULL) */
  int32_t mate_digit;        /* names ending in "/x" get the mate's digit (paired archives) */
  int32_t ignore_names;      /* -n: the name stream's mode byte is not consulted, names are <library>.<index> */
  int32_t split;             /* != 0: hand record_offsets to wr */
  const char *library;       /* with ignore_names: the library name to print */
  uint64_t window_text_bytes; /* 0: SCALCE_WINDOW_TEXT_DEFAULT */
  /* The length stream of a variable-length archive (PREFIX_<m>.scalcel out of its container, header included), a fourth
   * stream per mate; all NULL: an archive of reads of one length, as before.  Layout: the 8 magic bytes, int32 entry width
   * (1 if L <= 255, else 2), int32 L -- it must be the read stream's --, then one little-endian entry per record in archive
   * order: L - length.  Each window's records lose their pad on the device (scalce_fastq_strip_window) before they come down;
   * windows are still sized by their padded text.  A stream that ends before the records do: "(ERROR) truncated length
   * stream".  A range passes over first_record entries (len_skip, or reads that are dropped).  Not with interleave or
   * no_qualities (SCALCE_ERR_ARG). */
  scalce_read_fn len_rd[2];
  void *len_user[2];
  scalce_skip_fn len_skip[2];
  /* != 0: the text handed to wr is hashed on the device on its way out.  Each window's final text -- behind the records kernel,
   * exceptions, comments, pad strip and '+' lines -- or, with the order restore, each stripe's gathered text gets one
   * scalce_crc32_device launch on the buffer its download reads; the words come down beside the window's error words and are
   * joined in the order wr is called: stats->crc[m] / text_bytes[m] = zlib's crc32 and the size of everything wr received for
   * mate m (mates one after the other: [0], [1]; an interleaved text: [0]).  0: nothing of it is launched. */
  int32_t digest;
} scalce_unpack_params;
#define SCALCE_WINDOW_TEXT_DEFAULT (1ull << 30)
typedef int (*scalce_write_fn)(void *user, int mate, uint64_t first_record, uint64_t nrecords, const void *text,
                               uint64_t nbytes, const uint64_t *record_offsets);
typedef struct {
  uint64_t windows;            /* handed to wr */
  uint64_t window_text_bytes;  /* the bound in force */
  uint64_t peak_device_bytes;  /* sum of the session's own live device allocations, at its highest */
  uint64_t pinned_host_bytes;
  uint64_t records[2];         /* per mate (interleaved: pairs, in [0] and [1]) */
  double total_s, setup_s, read_wait_s, decode_s, records_s, write_wait_s, write_s;
                               /* read_wait: in rd; decode / records: device time of the kernels; write_wait: the session
                                  waiting for a window buffer that wr still holds; write: inside wr */
  int32_t error_mate, error_stream;  /* on failure: which stream of which mate (0 r, 1 n, 2 q, 3 l, 4 o, 5 c, 6 x, 7 p, 8 d), or -1 */
  int32_t error_wants_file;    /* the message in errbuf is a predicate: put the stream's file name in front of it */
  uint64_t decode_batches[2];  /* per mate: decoder batches enqueued (runs of whole frames, one scalce_ac_decoder_launch each) */
  uint32_t crc[2];             /* params->digest: see there */
  uint64_t text_bytes[2];
} scalce_unpack_stats;
int scalce_stream_decompress(scalce_ctx *ctx, const scalce_unpack_params *p, scalce_read_fn rd[2][3], void *user[2][3],
                             scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats, char *errbuf, size_t errcap);

/* A RANGE of records of the archive: records first_record .. first_record + nrecords - 1 in archive order, the order a whole
 * run writes them in (pairs for two mates: both mates take the same range, interleaved or one after the other).  The format
 * needs no index for it: what lies in front of the range is passed over stream by stream -- bucket headers are hopped (each
 * one is read and checked, the records behind it are not), mate 2's bare records, the raw quality rows of a -A archive and
 * whole frames of the coded quality stream (by their size words) are skipped, names are hopped by their length bytes -- and
 * only the frames that hold a symbol of the range are decoded: the first from its beginning, the symbols in front of the
 * range's first record are dropped, the last one up to the range's last symbol.  Nothing behind the range is read.
 * scalce_stream_decompress is this call with the range {0, ~0ull, no skips}; windows, buffers and wr are the same, and the
 * first_record handed to wr -- and the index of made-up names, <library>.<index> -- stays archive-absolute.
 * A first_record at or beyond the end gives no record and SCALCE_OK; nrecords is clamped to the end.  An archive that does
 * not say how many records it holds (no coded qualities) ends where the streams that end a whole run end.  A stream that
 * ends inside the part passed over, or inside the range, is the error it is for a whole run; A STREAM THAT ENDS BEHIND THE
 * RANGE IS NOT NOTICED.
 *   skip[m][k]   optional, per stream (0 r, 1 n, 2 q), called with the stream's `user`: passes over nbytes without delivering
 *                them (a plain file seeks).  Returns the bytes passed over (< nbytes: the stream ended there), < 0: error.
 *                NULL: the library reads through rd and drops the bytes (a gzip container).  The look-ahead buffer of a
 *                stream (SCALCE_UNPACK_LOOKAHEAD_BYTES) is used up before skip is called; the name stream is always read. */
#define SCALCE_UNPACK_LOOKAHEAD_BYTES (1u << 20)
typedef struct {
  uint64_t first_record;        /* zero-based, in archive order = the order -d writes; pairs for two mates */
  uint64_t nrecords;            /* ~0ull: to the end */
  scalce_skip_fn skip[2][3];    /* [mate][r, n, q], any of them NULL */
} scalce_unpack_range;
typedef struct {
  uint64_t first_record, nrecords;          /* the range in force after clamping to the archive */
  uint64_t total_records;                   /* ~0ull when the archive does not say (no coded qualities) */
  uint64_t frames_decoded[2], frames_passed[2], symbols_decoded[2];   /* per mate; symbols: what the decoder was launched
                                               for, the dropped ones in front included (the plan's out[2] + out[3]) */
  uint64_t bytes_delivered[2][3];           /* what rd handed over, dropped bytes included */
  uint64_t bytes_skipped[2][3];             /* what went through skip */
} scalce_unpack_range_stats;
int scalce_stream_decompress_range(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_range *range /* NULL: all */,
                                   scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                   scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats, char *errbuf, size_t errcap);
/* The range's arithmetic over the coded quality stream, no device call: records of read_len symbols, frames of
 * SCALCE_AC_BLOCK symbols, total_syms in the stream; first / n are clamped to its total_syms / read_len records.
 * out[0] = the first frame to decode (= frames passed over), out[1] = frames to decode (0 when the range is empty),
 * out[2] = symbols of frame out[0] in front of the range's first record (decoded and dropped), out[3] = symbols of the range
 * behind them -- n * read_len, plus the stream's trailing symbols (fewer than a record) when the range reaches the last record,
 * as a whole run decodes them.  The decoder is launched for out[2] + out[3] symbols. */
int scalce_range_plan_quality(int read_len, uint64_t first, uint64_t n, uint64_t total_syms, uint64_t out[4]);

/* ---- the input order back (archives made with --keep-order; kernels_restore.hpp, stream_decode.cpp) ---------------------
 * The order stream (PREFIX_1.scalceo out of its container): the 8 magic bytes, int32 4 (entry width), int32 0, int64 N, then
 * N little-endian u32 -- entry k is the input index of the k-th record (pair) of the archive, SCALCE_OUT_PERM.  On the way
 * back the records of a window belong at places spread over the whole output, so the output is cut into S STRIPES of R
 * consecutive input indices and the text travels twice: each window's records are grouped by stripe on the device and
 * appended to a spill; then, stripe by stripe, every window's share is read back, put in its places on the device and handed
 * to wr.  Memory follows the window; the text is written twice and read once.
 *
 * The device building blocks only enqueue on `stream`, allocate nothing and wait for nothing.
 *
 * scalce_records_permute: output record r is input record d_source[r] (an entry >= nrecords gives an empty record);
 *   d_out_offsets (nrecords + 1) is the scan of the permuted lengths.  d_text: any byte address; text_bytes: the bytes of
 *   d_text that hold the records (d_record_offsets[nrecords] <= text_bytes); d_out 16-byte aligned, nothing is stored at or
 *   past out_cap nor past the text's end; d_ws: scalce_records_permute_ws_bytes(nrecords) bytes.
 * scalce_order_group: d_source lists the window's records 0 .. nrecords - 1 grouped by stripe d_index[i] / stripe_records,
 *   stable within a stripe; d_stripe_counts[s] (nstripes entries, nstripes <= 65536) how many fell into stripe s; *d_bad is
 *   cleared, then set when an index is >= total_records (such a record is counted in the last stripe).  d_ws:
 *   scalce_order_group_ws_bytes(nrecords, nstripes) bytes.
 * scalce_order_place: d_source[d_index[i] - base] = i for the m records of a stripe (d_source: expect entries; a place that
 *   stays empty holds ~0); *d_bad is cleared, then set when an index lies outside [base, base + expect), when two records
 *   claim one place, or when a place stays empty.
 * scalce_order_gather: d_out[k] = d_in[d_source[k]], the order entries of the grouped records.
 * scalce_order_plan (no device call): out = {R, S}; R = max(1, window_text_bytes / max_record_bytes), raised where needed so
 *   that S = ceil(total_records / R) <= 65536. */
uint64_t scalce_records_permute_ws_bytes(uint64_t nrecords);
int scalce_records_permute(scalce_ctx *ctx, const uint8_t *d_text, const uint64_t *d_record_offsets, uint64_t nrecords,
                           uint64_t text_bytes, const uint32_t *d_source, uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_out_offsets, void *d_ws, void *stream);
uint64_t scalce_order_group_ws_bytes(uint64_t nrecords, uint64_t nstripes);
int scalce_order_group(scalce_ctx *ctx, const uint32_t *d_index, uint64_t nrecords, uint64_t stripe_records, uint64_t total_records,
                       uint64_t nstripes, uint32_t *d_source, uint32_t *d_stripe_counts, uint32_t *d_bad, void *d_ws, void *stream);
int scalce_order_place(scalce_ctx *ctx, const uint32_t *d_index, uint64_t m, uint64_t base, uint64_t expect, uint32_t *d_source,
                       uint32_t *d_bad, void *stream);
int scalce_order_gather(scalce_ctx *ctx, const uint32_t *d_in, const uint32_t *d_source, uint64_t n, uint32_t *d_out, void *stream);
int scalce_order_plan(uint64_t total_records, uint64_t window_text_bytes, uint64_t max_record_bytes, uint64_t out[2]);

/* scalce_stream_decompress with the input order restored.  order_rd[m] delivers the order stream, header included, once per
 * mate pass: two mates that are not interleaved go one after the other and each reads it from the start; interleaved, only
 * [0] is used and an entry counts pairs.  wr receives the text in INPUT order: first_record is the input index of the first
 * record handed over, a call holds one stripe.  spill_dir: where the two spill files are made (and unlinked at once).
 * Errors, besides those of scalce_stream_decompress: "(ERROR) truncated order stream", "(ERROR) is not a scalce order
 * stream", "(ERROR) order stream holds <n> entries, the archive <m> records", "(ERROR) order stream is not a permutation of
 * the records", and a spill file that cannot be made or written (error_stream 4 names the order stream). */
typedef struct {
  scalce_read_fn order_rd[2];
  void *order_user[2];
  const char *spill_dir;
} scalce_restore_params;
typedef struct {
  uint64_t records;         /* restored (per mate pass: the archive's records or pairs) */
  uint64_t stripes;         /* S */
  uint64_t stripe_records;  /* R */
  uint64_t spilled_bytes;   /* text and record words written to the spill, all mate passes */
  double group_pass_s;      /* wall time of the window loop (decode, group, spill) */
  double stripe_pass_s;     /* wall time of the stripe loop (read back, place, write) */
  double spill_write_s, spill_read_s;  /* inside write(2) / pread(2) on the spill files */
  double place_wait_s;      /* the stripe loop waiting for the device (upload, place, permute, download) */
} scalce_restore_stats;
int scalce_stream_decompress_restore(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_restore_params *rp,
                                     scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                     scalce_unpack_stats *stats, scalce_restore_stats *restore_stats, char *errbuf, size_t errcap);

/* ---- what follows the names, back on the way out (archives made with --keep-comments; commentstream.hpp, kernels_comments.hpp) ---
 * The comment stream (PREFIX_<m>.scalcec out of its container), one per mate: the 8 magic bytes, int32 0 (entry width 0: text
 * entries), int32 C (the longest entry in bytes, without its terminator), int64 N, then N entries in archive order, each followed
 * by a newline: SCALCE_OUT_COMMENTS.  com_rd[m] delivers mate m's, header included; both NULL: no comments.  Every record's entry
 * is taken with its name and counts in the window's budget: a window holds at most window_text_bytes of text WITH its entries,
 * and device and pinned memory follow the window (a record's bound grows by C), never C x records.  Each window's entries go
 * back on the device (scalce_fastq_comment_window) before the pad goes (variable-length archives) and before the order restore
 * groups the window.  A range passes over first_record entries by their newlines; the stream is always read.
 * scalce_stream_decompress_comments covers the three shapes of decompression: range and rp NULL is scalce_stream_decompress,
 * range set scalce_stream_decompress_range, rp set scalce_stream_decompress_restore (both: SCALCE_ERR_ARG); comments NULL is the
 * existing call of that shape.  Every mate has its stream (else SCALCE_ERR_ARG); interleaved, both mates' entries of a window go
 * into its one text (scalce_fastq_comment_window_pairs).  Not for an archive without stored names.  Errors besides theirs: "(ERROR) truncated comment stream" (it ends inside an entry or before the
 * records do), "(ERROR) is not a scalce comment stream", "(ERROR) comment stream holds <n> entries, the archive <m> records",
 * "(ERROR) comment stream: an entry is longer than its header says"; error_stream 5 names the comment stream. */
typedef struct {
  scalce_read_fn com_rd[2];
  void *com_user[2];
} scalce_unpack_comments;
int scalce_stream_decompress_comments(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments,
                                      const scalce_unpack_range *range /* NULL: all */, const scalce_restore_params *rp /* NULL: archive order */,
                                      scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user,
                                      scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats,
                                      scalce_restore_stats *restore_stats, char *errbuf, size_t errcap);

/* ---- the letters and qualities the archive does not keep, back on the way out (archives made with --keep-bases; exceptionstream.hpp,
 * kernels_exceptions.hpp) -----
 * The exception stream (PREFIX_<m>.scalcex out of its container), one per mate: the 8 magic bytes, int32 8 (entry width), int32 L,
 * int64 N (records), int64 X (entries), then X little-endian u64 in strictly ascending order: SCALCE_OUT_EXCEPTIONS (bits 0-7 the
 * letter, 8-15 the quality character, 16-27 the position, 28-63 the record's index in archive order; pairs: the pair's index, each
 * mate in its own stream with its own L).  What it undoes: getval stores a c g t as A C G T and every other letter as A (const.h:127,
 * const.cpp:47-49), an N forces quality symbol 0 (qualities.cpp:183) and every symbol 0 comes back as N (decompress.cpp:350-351).
 * exc_rd[m] delivers mate m's, header included; both NULL: no exceptions.  Each window takes the entries of its records over the
 * callback -- a range passes over those in front of it and reads none behind it, memory follows the window's entries -- and they go
 * back on the device (scalce_fastq_exception_window) directly behind the records kernel: before the comments go back, the pad goes
 * and the order restore groups the window.  Without qualities on the way out (-Q) only the letters are written.
 * scalce_stream_decompress_exceptions is scalce_stream_decompress_comments with the exception streams beside the comment streams;
 * either may be NULL, range and rp as there.  Every mate has its stream (else SCALCE_ERR_ARG).  Errors besides theirs: "(ERROR)
 * truncated exception stream", "(ERROR) is not a scalce exception stream", "(ERROR) exception stream holds <n> records, the archive
 * <m>", "(ERROR) exception stream is for reads of <l> bases, the archive's have <L>", "(ERROR) exception stream: entries are not in
 * ascending order", "(ERROR) exception stream: an entry lies outside its record"; error_stream 6 names the exception stream. */
typedef struct {
  scalce_read_fn exc_rd[2];
  void *exc_user[2];
} scalce_unpack_exceptions;
int scalce_stream_decompress_exceptions(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments /* NULL: none */,
                                        const scalce_unpack_exceptions *exceptions /* NULL: none */, const scalce_unpack_range *range /* NULL: all */,
                                        const scalce_restore_params *rp /* NULL: archive order */, scalce_read_fn rd[2][3], void *user[2][3],
                                        scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats, scalce_unpack_range_stats *range_stats,
                                        scalce_restore_stats *restore_stats, char *errbuf, size_t errcap);

/* ---- the '+' lines, back on the way out (archives made with --keep-plus; plusstream.hpp, kernels_plus.hpp) -----------------
 * The plus-line stream (PREFIX_<m>.scalcep out of its container), one per mate: the 8 magic bytes, int32 0 (text entries, as in
 * .scalcec), int32 P (the longest stored entry in bytes), int64 N, then N entries in archive order, each followed by a newline:
 * SCALCE_OUT_PLUS.  P = 0: no entries follow, every record's line is bare.  plus_rd[m] delivers mate m's, header included; both
 * NULL: no such streams.
 *
 * scalce_fastq_plus_window mirrors scalce_fastq_comment_window and runs BEHIND it and behind scalce_fastq_strip_window (both
 * measure from the record's end and assume "\n+\n" between bases and qualities): d_text / d_record_offsets are a window's
 * records of any header and read length (nrecords + 1 offsets; records with qualities), d_entries its entry_bytes bytes of the
 * stream: nrecords entries, each followed by a newline, found on the device by a newline index.  A repeat grows its record by
 * the header line as the text holds it (comments included when they were put back), a literal by its bytes.  d_out (out_cap
 * bytes of room) receives the text, d_out_offsets (nrecords + 1) where each record begins in it and, last, its size.  *d_bad is
 * set when the entries do not hold exactly nrecords newlines, when an entry's first byte is neither '=' nor '\'' or a '=' has
 * bytes behind it (such records get a bare '+'), or when the text would outgrow out_cap (nothing is written then).  d_text,
 * d_entries and d_out 16-byte aligned; d_ws: scalce_fastq_plus_ws_bytes(nrecords, entry_bytes) bytes.  Enqueued on `stream`;
 * allocates nothing, waits for nothing.  _pairs mirrors scalce_fastq_comment_window_pairs: an interleaved window of npairs
 * pairs of read_len[0] / read_len[1] bases; d_entries: 2 npairs entries, mate 1's then mate 2's of each pair.
 *
 * scalce_stream_decompress_plus is scalce_stream_decompress_exceptions with the plus-line streams beside the others; each may be
 * NULL, range and rp as there.  Every mate has its stream (else SCALCE_ERR_ARG).  A record's entry is taken with the record and
 * counts in the window's budget with what it adds to the text: the bound of a record's text grows by max(P - 1, the bound of
 * its header line), device and pinned memory follow the window.  A range passes over the entries in front of it and reads none
 * behind it.  Not with params no_qualities (two-line records have no such line: SCALCE_ERR_ARG).  Errors besides theirs:
 * "(ERROR) truncated plus-line stream", "(ERROR) is not a scalce plus-line stream", "(ERROR) plus-line stream holds <n> entries,
 * the archive <m> records", "(ERROR) plus-line stream: an entry is longer than its header says", "(ERROR) plus-line stream:
 * malformed entry"; error_stream 7 names the plus-line stream. */
uint64_t scalce_fastq_plus_ws_bytes(uint64_t nrecords, uint64_t entry_bytes);
int scalce_fastq_plus_window(scalce_ctx *ctx, uint64_t nrecords, const uint8_t *d_text, const uint64_t *d_record_offsets,
                             const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                             uint32_t *d_bad, void *d_ws, void *stream);
uint64_t scalce_fastq_plus_pairs_ws_bytes(uint64_t npairs, uint64_t entry_bytes);
int scalce_fastq_plus_window_pairs(scalce_ctx *ctx, const int read_len[2], uint64_t npairs, const uint8_t *d_text,
                                   const uint64_t *d_pair_offsets, const uint8_t *d_entries, uint64_t entry_bytes, uint8_t *d_out,
                                   uint64_t out_cap, uint64_t *d_out_pair_offsets, uint32_t *d_bad, void *d_ws, void *stream);
typedef struct {
  scalce_read_fn plus_rd[2];
  void *plus_user[2];
} scalce_unpack_plus;
int scalce_stream_decompress_plus(scalce_ctx *ctx, const scalce_unpack_params *p, const scalce_unpack_comments *comments /* NULL: none */,
                                  const scalce_unpack_exceptions *exceptions /* NULL: none */, const scalce_unpack_plus *plus /* NULL: none */,
                                  const scalce_unpack_range *range /* NULL: all */, const scalce_restore_params *rp /* NULL: archive order */,
                                  scalce_read_fn rd[2][3], void *user[2][3], scalce_write_fn wr, void *wr_user, scalce_unpack_stats *stats,
                                  scalce_unpack_range_stats *range_stats, scalce_restore_stats *restore_stats, char *errbuf, size_t errcap);

/* ---- runs sharded over several GPUs: one process per GPU, ONE archive -----------------------------------------
 * The reference has no distributed mode; what it carries across reads is what ranks exchange (see comm.cpp).  The
 * archive of a sharded run is byte for byte the archive of the same input on one GPU -- and of the reference at -T 1 with
 * the same -B -- for any number of ranks: rank boundaries are moved to the nearest spill-chunk boundary of the run-wide -B
 * rule (records change owner as text, once), so that "rank-major inside a bucket" IS the merge order of compress.cpp:104-159.
 * -B must be set (the reference's default is 4G).  Ranks whose share is smaller than a chunk may end up without records; a
 * run that -B does not cut at all is ONE chunk, whose rows all go to rank 0 (scalce_shard_plan_boundaries). */
typedef struct scalce_comm scalce_comm;
#define SCALCE_COMM_ID_BYTES 128
int scalce_comm_unique_id(uint8_t id[SCALCE_COMM_ID_BYTES]);  /* rank 0 makes it, the launcher hands it to every rank */
int scalce_comm_create_rccl(int device, int world, int rank, const uint8_t id[SCALCE_COMM_ID_BYTES], scalce_comm **out);
/* rehearsal transport: `world` processes sharing one GPU, staged through POSIX shared memory `name` (slot_bytes per rank,
 * 0 = 64 MiB: the largest message) */
int scalce_comm_create_shm(int device, int world, int rank, const char *name, uint64_t slot_bytes, scalce_comm **out);
void scalce_comm_destroy(scalce_comm *c);
const char *scalce_comm_error(const scalce_comm *c);
int scalce_comm_world(const scalce_comm *c);
int scalce_comm_rank(const scalce_comm *c);
/* Largest message handed to the transport in one piece (default 1 GiB: RCCL loses the tail of larger ones between a rank and
 * itself, comm.cpp); tools/rccl_big_send.py raises it to show where. */
void scalce_comm_set_piece_bytes(scalce_comm *c, uint64_t bytes);
int scalce_comm_barrier(scalce_comm *c, void *stream);
int scalce_comm_all_gather(scalce_comm *c, const void *d_send, void *d_recv, uint64_t bytes_per_rank, void *stream);
int scalce_comm_all_reduce_sum_u64(scalce_comm *c, uint64_t *d_buf, uint64_t count, void *stream);
/* One message between two ranks (what a chain of ranks hands on: the counts of the tie-break, rank r to rank r + 1). */
int scalce_comm_send(scalce_comm *c, const void *d_buf, uint64_t bytes, int peer, void *stream);
int scalce_comm_recv(scalce_comm *c, void *d_buf, uint64_t bytes, int peer, void *stream);
int scalce_comm_all_to_all_v(scalce_comm *c, const void *d_send, const uint64_t *send_bytes, void *d_recv,
                             const uint64_t *recv_bytes, void *stream);
/* The same with explicit offsets: the bytes for rank d start at d_send + send_off[d], those from rank src land at
 * d_recv + recv_off[src] -- a rank sends ranges of a buffer where they lie and keeps its own part out of the transport. */
int scalce_comm_all_to_all_vo(scalce_comm *c, const void *d_send, const uint64_t *send_off, const uint64_t *send_bytes,
                              void *d_recv, const uint64_t *recv_off, const uint64_t *recv_bytes, void *stream);

typedef struct {
  int32_t world, rank;
  uint32_t nb1;              /* buckets + 1 (root last) */
  uint32_t rounds;           /* collective rounds of the tie-break */
  uint32_t sweeps;           /* local sweeps of this rank */
  uint32_t chunks_total;     /* spill chunks of the run */
  uint64_t reads_total;      /* of the run */
  uint64_t first_read;       /* run-wide index of this rank's first record AFTER the boundaries moved */
  uint64_t reads_local;      /* records this rank holds after the move */
  uint64_t moved_in[2];      /* records received from the rank before / behind */
  uint64_t *counts;          /* [world][nb1] reads per (rank, bucket), emission order */
  uint64_t *name_bytes;      /* [world][nb1] bytes of their name records */
  uint64_t sym_lo[2], sym_hi[2];  /* per mate: this rank's range of the run-wide reordered quality stream (whole 10 MiB blocks) */
  uint64_t coded_bytes[2][64];    /* per mate and rank: bytes of framed blocks (0 with SCALCE_SHARD_PREPARE_ONLY) */
  void *keep[8];             /* device buffers the coder still reads (freed by scalce_shard_result_free) */
  uint64_t keep_bytes[8];
  uint32_t magic;            /* set by the library: a result handed back in keeps its buffers */
} scalce_shard_result;
#define SCALCE_SHARD_PREPARE_ONLY 1  /* hand the rank's block range to the batch (scalce_batch_entropy_stream_prepare): the
                                        caller codes several shards with one scalce_batch_entropy_begin_group */
#define SCALCE_SHARD_CODER_ASYNC 2   /* only enqueue the coder on coder_stream (scalce_batch_entropy_stream_begin) */
/* SPMD: every rank calls it with its own contiguous piece of the read stream (rank order = input order), resident in
 * HBM.  On return the batch holds this rank's pieces of the archive: SCALCE_OUT_READS / _NAMES = its records per bucket
 * (bucket b of the archive = header, then rank 0's records of b, rank 1's, ...: result->counts / name_bytes say where),
 * SCALCE_OUT_QUAL = the framed blocks of sym_lo .. sym_hi, SCALCE_OUT_TABLE = the run-wide table.  `b` must have been
 * created with bucket_set_size != 0 and default qprev.  `result` must be zeroed before its first use; handing the result
 * of an earlier call on the same batch back in reuses its device buffers (no allocation, hence no device-wide
 * synchronisation, in the steady state of a pipeline). */
int scalce_sharded_compress(scalce_comm *comm, scalce_ctx *ctx, scalce_batch *b, const uint8_t *d_text1, uint64_t n1,
                            const uint8_t *d_text2, uint64_t n2, int flags, void *stream, void *coder_stream,
                            scalce_shard_result *result);
void scalce_shard_result_free(scalce_shard_result *r);
/* The host-side plan math of a sharded run on its own (no device needed; see sharded.cpp): rank boundaries g[0..world]
 * moved to the nearest cut of the run-wide -B rule; the deal of the run-wide reordered quality stream in contiguous
 * ranges of whole 10 MiB blocks; the trigram counters (p0 * 80 + p1) * 80 + s that straddle the boundary in front of a
 * rank's original piece (nsym[r] symbols per rank, edges + r * edge_stride = its scalce_batch_qinput_edges); and the
 * pieces of _plan_blocks split into those that read the local stream (own_src relative to *local_off) and those that
 * read a receive buffer holding only what other ranks sent.  SCALCE_ERR_ARG on arguments or a plan that make no sense. */
int scalce_shard_plan_boundaries(int world, const uint64_t *g, const uint64_t *cuts_sorted, uint64_t ncuts, uint64_t *gn);
int scalce_shard_plan_blocks(int world, int rank, uint32_t nb1, const uint64_t *counts /*[world][nb1]*/, uint64_t read_len,
                             uint64_t *send_bytes, uint64_t *recv_bytes, uint64_t *lo, uint64_t *hi, uint64_t *piece_src,
                             uint64_t *piece_dst, uint64_t *npieces);
int scalce_shard_plan_edge_trigrams(int world, int rank, const uint64_t *nsym /*[world]*/, const uint8_t *edges, uint64_t edge_stride,
                                    uint32_t keys[2], uint32_t *nkeys);
int scalce_shard_plan_own_pieces(int world, int rank, const uint64_t *send_bytes, const uint64_t *recv_bytes, const uint64_t *piece_src,
                                 const uint64_t *piece_dst, uint64_t npieces, uint64_t *own_src, uint64_t *own_dst, uint64_t *nown,
                                 uint64_t *own_total, uint64_t *local_off, uint64_t *other_src, uint64_t *other_dst, uint64_t *nother,
                                 uint64_t *other_total);

/* ---- shards in flight (pipeline.cpp) -----------------------------------------------------------------------------
 * The reference keeps its cores busy by handing -T blocks of a batch to coder threads while the reader goes on
 * (arithmetic.cpp:349-357, compress.cpp:781-786).  The device-side counterpart for a caller with MANY shards: `nslots`
 * batches (usually sharing one scalce_workspace), the front stages (scalce_batch_ingest .. _emit) of the next shards on one
 * stream beside the coder launches of the previous ones on `coder_streams` others, `group` shards per coder launch
 * (nslots >= 2 * group for launches that go out as they fill up), a shard retired on an event behind its launch.
 * external_coder != 0: the caller enqueues or prepares the coder itself (scalce_sharded_compress with
 * SCALCE_SHARD_CODER_ASYNC / _PREPARE_ONLY).
 *     for every shard:  scalce_pipeline_acquire(p, &slot, &retired);   (retired: take the outputs of the shard that was there)
 *                       ... front stages of the shard into batches[slot] on scalce_pipeline_front_stream(p) ...
 *                       scalce_pipeline_submit(p, slot, flush_now, &launched);
 *     scalce_pipeline_drain(p);          (the caller walks the slots for their outputs, or retires them one by one before)
 * flush_now: 0 = the launch goes out when `group` shards are pending; 1 = what is pending goes out now and nothing will run
 * beside it (the end of a run, or a wave that fills every slot -- `group` may be as large as nslots, up to SCALCE_GROUP_MAX,
 * for a caller that plans its launches): it is shaped for its own latency, on every CU; 2 = it goes out now, front stages of
 * further shards follow beside it.  A coder launch takes ~0.5 s whether it holds five 50 M-read shards or fifteen: a caller that knows the length
 * of its run puts the remainder first and then launches whole waves (bench.py --launch-plan waves). */
typedef struct scalce_pipeline scalce_pipeline;
int scalce_pipeline_create(scalce_batch **batches, int nslots, int group, int coder_streams, int external_coder, scalce_pipeline **out);
void scalce_pipeline_destroy(scalce_pipeline *p);
const char *scalce_pipeline_error(const scalce_pipeline *p);
void *scalce_pipeline_front_stream(scalce_pipeline *p);
void *scalce_pipeline_coder_stream(scalce_pipeline *p, int i);
int scalce_pipeline_acquire(scalce_pipeline *p, int *slot, int *retired);
int scalce_pipeline_submit(scalce_pipeline *p, int slot, int flush_now, int *launched);
int scalce_pipeline_retire(scalce_pipeline *p, int slot, int *had_shard);
int scalce_pipeline_flush_last(scalce_pipeline *p);  /* what is pending goes out as the last launch of a run */
int scalce_pipeline_drain(scalce_pipeline *p);

#ifdef __cplusplus
}
#endif
#endif /* SCALCE_HIP_H */
