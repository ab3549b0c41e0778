// cli.cpp -- `scalce`: command-line drop-in for the reference's process contract
// (/root/reference/main.cpp:187-303, HELP) over libscalce_hip.so.
//
//   scalce [opts] -o PREFIX in_1.fastq[.gz] ...     ->  PREFIX_1.scalce{n,r,q} (+ PREFIX_2.* with -r)
//   scalce X_1.scalcen -d -o OUT                    ->  OUT_1.fastq (+ OUT_2.fastq)
//
// Host side only: option parsing, file I/O (plain / gzip via zlib), the quality sample
// (quality_mapping_init's read loop, qualities.cpp:64-97), the file headers of
// combine_and_compress_with_split (compress.cpp:289-343) and, for -d, the record loop of
// decompress.cpp:259-369.  Every byte of the hot path is produced by the HIP kernels; there is no CPU
// fallback -- without a GPU the tool stops with an error.
//
// What needs HIP or the library is here: the downloads, the archive headers, the quality model, the three runs and main().
// The host logic between them has headers of its own, which compile without HIP (tools/cli_host_check.cpp drives them):
//   cli_io.hpp      messages, thread counts, Fd, parallel reads, line counting, OutFile
//   cli_input.hpp   MateSource (a mate's files joined), sample_stats
//   cli_shares.hpp  --gpus: a rank's record range (LineRanges), its share of every bucket (Shares, place_share)
//   cli_sink.hpp    -d: ArchiveFile behind the read callbacks, TextSink behind the write callback
#include <getopt.h>
#include <hip/hip_runtime_api.h>
#include <sys/wait.h>

#include <cerrno>
#include <csignal>

#include "../../include/scalce_hip.h"
#include "hip_own.hpp"
#include "digeststream.hpp"
#include "cli_io.hpp"
#include "cli_input.hpp"
#include "cli_shares.hpp"
#include "cli_sink.hpp"
#include "cli_sidefiles.hpp"

#ifndef SCALCE_VERSION
#define SCALCE_VERSION "2.8-mi355x"
#endif

struct Options {
  int lossy = 0, sample = 100000, threads = 0, split = 0;
  bool paired = false, use_names = true, no_ac = false, decompress = false;
  bool fasta = false, no_qual = false;    // -f (implies no qualities, main.cpp:220-223), -Q (main.cpp:270-272)
  bool interleave = false;                // -i: pairs in ONE file, mate 1 then mate 2 (main.cpp:196,225, commented out there)
  bool pairs() const { return paired || interleave; }  // two mates, whichever way they come in
  uint64_t bucket_set_size = 4ull << 30;  // main.cpp:68
  std::string out, library, patterns, temp = "__temp__", patterns_bin;
  uint64_t window = 0;                    // --window: bytes of FASTQ text per decompression window (0: the library's default)
  bool has_range = false;                 // --records FIRST[:COUNT]: decompress this range of records (pairs) only
  uint64_t range_first = 0, range_count = ~0ull;
  bool varlen = false;                    // --variable-length: reads of 0 .. L bases, padded to L on the device, lengths in PREFIX_<m>.scalcel
  int max_length = 0;                     // --max-length NUM: L given, not taken from the sample (implies --variable-length)
  bool keep_order = false;                // --keep-order: the input index of every record of the archive, in PREFIX_1.scalceo
  bool archive_order = false;             // -d --archive-order: a .scalceo next to the archive is ignored
  bool keep_comments = false;             // --keep-comments: what follows every record's name, in PREFIX_<m>.scalcec
  bool no_comments = false;               // -d --no-comments: a .scalcec next to the archive is ignored
  bool keep_plus = false;                 // --keep-plus: what stood on every record's '+' line, in PREFIX_<m>.scalcep
  bool bare_plus = false;                 // -d --bare-plus: a .scalcep next to the archive is ignored
  bool lossless = false;                  // --lossless: --keep-order --keep-comments --keep-bases --keep-plus (-f: without the last)
  bool keep_bases = false;                // --keep-bases: every letter and quality the archive does not keep, in PREFIX_<m>.scalcex
  bool stored_bases = false;              // -d --stored-bases: a .scalcex next to the archive is ignored
  bool digest = false;                    // --digest (with --lossless): bytes and CRC-32 of every input text, in PREFIX_1.scalced
  bool test = false;                      // -d --test: decode everything, check the digest, write nothing
  bool temp_given = false;                // -t was given (the default of `temp` is the reference's)
  int gpus = 1;                           // --gpus N: one process per GPU, ONE archive (plain-text input, -c no)
  int container = 1;                      // 0 plain, 1 gzip (main.cpp:181-184 at -T 1)
  uint64_t first_file_bytes[2] = {0, 0};  // --gpus over several files written out as one: where the first file ends (the
                                          // quality sample never leaves files[0], compress.cpp:761)
};

static const char *HELP_TEXT =
    "SCALCE " SCALCE_VERSION " (MI355X hot path)\n"
    "usage: scalce [options] -o OUTPUT FILE_1.fastq[.gz] ...      compress\n"
    "       scalce FILE_1.scalcen -d -o OUTPUT                   decompress\n"
    "  -o, --output STR            output prefix (required)\n"
    "  -r, --paired-end            FILE_1 is paired with the file whose last '1' is a '2'\n"
    "  -i, --interleave            paired-end reads interleaved in one file (mate 1, then mate 2 of every pair; each input\n"
    "                              file holds whole pairs).  The archive is the one -r makes of the two mates split into _1 / _2\n"
    "                              files: names are mate 1's as -r stores them (a trailing /1 is NOT stripped).  Decompression:\n"
    "                              one interleaved FASTQ (OUTPUT_1.fastq, or -o - for stdout; -S counts pairs).  One GPU only\n"
    "  -n, --skip-names STR        drop read names, regenerate them as STR.<index>\n"
    "  -c, --compression STR       container of the read/name streams: gz (default), pigz (= gz), no; bz is not built\n"
    "  -A, --no-arithmetic         store qualities raw instead of arithmetic coding\n"
    "  -f, --fasta                 input is FASTA (a name line and one sequence line per record): no qualities are stored\n"
    "  -Q, --no-qualities          drop the qualities of FASTQ input; decompression: write two-line records (@name, bases)\n"
    "                              of an archive made with -Q or -f (bases stored as N come back as A).  One GPU only\n"
    "      --variable-length       reads of different lengths (trimmed FASTQ): every read is padded with N to the longest read\n"
    "                              of the quality sample and its length kept in OUTPUT_<m>.scalcel; the other files are those\n"
    "                              of the padded reads.  Decompression finds the .scalcel by itself.  Not with -i, -f, -Q, --gpus\n"
    "      --max-length NUM        the longest read, when the sample may not hold it (implies --variable-length)\n"
    "      --keep-order            keep the order of the input: the input index of every record (pair) of the archive goes into\n"
    "                              OUTPUT_1.scalceo, every other file is the one the run without the option writes.  Decompression\n"
    "                              finds the .scalceo by itself and writes the records in the order they came in.  Not with --gpus\n"
    "      --archive-order         decompression: ignore the .scalceo, write the records in the archive's order\n"
    "      --keep-comments         keep what follows the name on every record's header line (from the first space on: mate number,\n"
    "                              barcode, length=...): it goes into OUTPUT_<m>.scalcec, every other file is the one the run\n"
    "                              without the option writes.  Decompression finds the .scalcec by itself and puts the comments\n"
    "                              back; the '+' line stays a bare '+'.  Not with -n, --gpus\n"
    "      --no-comments           decompression: ignore the .scalcec, write the names alone\n"
    "      --keep-plus             keep every record's third line: a bare '+', a repeat of the header line, or a line of its own goes\n"
    "                              into OUTPUT_<m>.scalcep, every other file is the one the run without the option writes.\n"
    "                              Decompression finds the .scalcep by itself and puts the lines back.  Not with -f, -Q, --gpus\n"
    "      --bare-plus             decompression: ignore the .scalcep, write a bare '+'\n"
    "      --lossless              --keep-order --keep-comments --keep-bases --keep-plus: scalce -d returns the input byte for\n"
    "                              byte.  Not with -p above 0, -n, -Q, --gpus\n"
    "      --digest                with --lossless: the size and zlib's CRC-32 of every input text (one per mate stream: several\n"
    "                              files are their concatenation, gzip input is its decompressed text) go into OUTPUT_1.scalced,\n"
    "                              taken on the device as the text comes up; every other file is the one the run without the\n"
    "                              option writes.  For one single-member .fastq.gz the number is the one gzip -lv prints.\n"
    "                              Decompression finds the .scalced by itself, takes the same number of the text it writes and\n"
    "                              ends with status 1 when they differ (the output stays); it is not checked when another text\n"
    "                              than the input's was asked for (--archive-order, --no-comments, --stored-bases, --bare-plus,\n"
    "                              -n, -Q, --records, -i for -r's archive or -r for -i's, a stream of --lossless missing)\n"
    "      --test                  decompression: decode everything and check the digest, write nothing (-o is not needed);\n"
    "                              status 0: every stream read to its end without error and, with a .scalced, the text matches\n"
    "      --keep-bases            keep every base letter and the quality under an N: the archive stores a c g t as A C G T, every\n"
    "                              other letter as A, an N only through its quality, and returns a base whose quality maps to the\n"
    "                              lowest as N.  What it changes goes into OUTPUT_<m>.scalcex, every other file is the one the\n"
    "                              run without the option writes.  Decompression finds the .scalcex by itself and puts the letters\n"
    "                              and qualities back.  Not with --gpus\n"
    "      --stored-bases          decompression: ignore the .scalcex, write the bases as the archive stores them\n"
    "  -p, --lossy-percentage INT  lossy quality transform, 0..100 (default 0)\n"
    "  -s, --sample-size INT       records sampled for the quality model (default 100000)\n"
    "  -B, --bucket-set-size NUM[M|G]  bucket storage that triggers a spill chunk (default 4G); order follows the reference\n"
    "  -P, --patterns FILE         text list of cores instead of the built-in table\n"
    "  -T, --threads INT           host threads that read plain input and deflate the gz containers (default: cores - 1,\n"
    "                              at most 64);\n"
    "                              the hot path itself runs on the GPU\n"
    "  -t, --temp-directory STR    where decompression spills while it restores the input order (two unnamed files; default:\n"
    "                              the directory of OUTPUT, or $TMPDIR for -o -) and where --gpus writes joined input files\n"
    "  -S, --split-reads INT       decompression: reads per output part\n"
    "      --window NUM[K|M|G]     decompression: bytes of FASTQ text per window (default 1G; -Q counts a record as its FASTQ).  The archive moves through the\n"
    "                              device in windows of whole records -- at least one record each --, so memory follows the\n"
    "                              window, not the archive, and -o - writes each window as it arrives\n"
    "      --records FIRST[:COUNT] decompression: only COUNT records (pairs under -r / -i; to the end without COUNT) from record\n"
    "                              FIRST on, counted from 0 in the order -d writes them.  What lies in front is passed over, not\n"
    "                              decoded (plain files seek); -S parts and made-up names (-n) count from FIRST; a file that\n"
    "                              is cut short behind the range is not noticed.  Counts in the archive's order: with a .scalceo\n"
    "                              next to the archive it needs --archive-order\n"
    "  -d, --decompress    -v, --version    -h, --help\n"
    "      --gpus N                compress on N GPUs, one process each, into ONE archive that is byte for byte the archive of\n"
    "                              one GPU (and of the reference at -T 1 with the same -B); input: one plain FASTQ file (pair), -c no\n"
    "core table: --patterns-bin FILE or $SCALCE_PATTERNS or patterns.bin next to the executable\n";

// ---- the archive: the file headers of combine_and_compress_with_split (compress.cpp:263-343) ---------------------------
//   PREFIX_<m>.scalcer  magic, int32 no_ac (-A), int32 read length; the read stream (mate 1: buckets, each opened by
//                       [int32 core][int64 records]; mate 2: bare records in mate 1's order)
//   PREFIX_<m>.scalcen  magic, u8 names; the name stream, or without names (-n) int64 0 and the library name
//   PREFIX_<m>.scalcel  --variable-length only (lenstream.hpp): magic, int32 entry width, int32 L, one entry L - length per record
//   PREFIX_1.scalceo    --keep-order only (orderstream.hpp): magic, int32 4, int32 0, int64 N, N x u32: the input index of the
//                       k-th record (pair) of the archive; one file for both mates
//   PREFIX_<m>.scalcec  --keep-comments only (commentstream.hpp): magic, int32 0, int32 C (longest entry), int64 N, then what follows
//                       the name of each record of the archive, from the first space on, each entry followed by a newline
//   PREFIX_<m>.scalcex  --keep-bases only (exceptionstream.hpp): magic, int32 8, int32 L, int64 N, int64 X, then X x u64 in ascending
//                       order: letter | quality character << 8 | position << 16 | record of the archive << 28
//   PREFIX_<m>.scalcep  --keep-plus only (plusstream.hpp): magic, int32 0, int32 P (longest stored entry), int64 N, then the '+' line
//                       of each record of the archive as an entry (empty: bare, '=': the header line again, '\'' + the line's
//                       bytes), each followed by a newline; P = 0: no entries
//   PREFIX_1.scalced    --digest only (digeststream.hpp): magic, int32 16, int32 kind (0 one text, 1 paired files, 2 interleaved; + 4
//                       two-line records), int64 T, then T x {u64 bytes, u32 crc32, u32 0}: each input text's size and zlib CRC-32
//   PREFIX_<m>.scalceq  magic, int64 Phred offset (mate 1's for both mates, compress.cpp:294,816-817); arithmetic coded:
//                       the scaled table (QTABLE_WORDS x u32), the int64 symbol count and the coded blocks; -A: the q' rows
static constexpr size_t QTABLE_WORDS = 512000;
static std::string archive_path(const std::string &out, int m, char ext) { return out + "_" + std::to_string(m + 1) + ".scalce" + ext; }
// fn(extension, path) on every mate's files with the extensions `exts` ("rnq": .scalcer, .scalcen, .scalceq)
template <class Fn> static void for_each_archive_file(const Options &o, const char *exts, Fn fn) {
  for (int m = 0; m < (o.pairs() ? 2 : 1); m++)
    for (const char *e = exts; *e; e++) fn(*e, archive_path(o.out, m, *e));
}
// -c gz holds every file in a gzip container but an arithmetic-coded .scalceq (compress.cpp:249)
static bool gz_container(const Options &o, char ext) { return o.container == 1 && (ext != 'q' || o.no_ac); }
static std::vector<uint8_t> with_magic(const void *fields, size_t n) {
  std::vector<uint8_t> h(scalce_host::ARCHIVE_MAGIC, scalce_host::ARCHIVE_MAGIC + 8);
  h.insert(h.end(), static_cast<const uint8_t *>(fields), static_cast<const uint8_t *>(fields) + n);
  return h;
}
static std::vector<uint8_t> reads_header(const Options &o, int len) { const int32_t f[2] = {o.no_ac, len}; return with_magic(f, 8); }
static std::vector<uint8_t> names_header(const Options &o) {  // without names: the whole file
  const uint8_t un = o.use_names ? 1 : 0;
  std::vector<uint8_t> h = with_magic(&un, 1);
  if (!o.use_names) { h.resize(h.size() + 8, 0); h.insert(h.end(), o.library.begin(), o.library.end()); }
  return h;
}
static std::vector<uint8_t> qual_header(int64_t phred) { return with_magic(&phred, 8); }

#define HIPOK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) FAIL("%s: %s\n", #x, hipGetErrorString(e_)); } while (0)
#define SCOK(ctx, x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s\n", scalce_last_error(ctx)); exit(1); } } while (0)

static std::vector<uint8_t> fetch(scalce_ctx *ctx, scalce_batch *b, int which, int mate) {
  const void *d = nullptr;
  uint64_t n = 0;
  SCOK(ctx, scalce_batch_output(b, which, mate, &d, &n));
  std::vector<uint8_t> v((size_t)n);
  if (n) SCOK(ctx, scalce_memcpy_d2h(ctx, v.data(), d, n));
  return v;
}

// A device stream to a file: slices come down into two pinned buffers in turn, the write (or deflate) of one slice runs
// while the next is on its way.  ONE writer per file: write(2) to tmpfs moves 6 GB/s from one thread on the bench host and
// holds the inode's lock -- four threads with a slice each and pwrite at the slices' offsets measured 0.9 s against 0.5 for
// the 1.9 GB of a quality stream, threads copying into a shared mapping 3-4 GB/s (tools/write_bench.cpp).  The framing
// kernel's stores into the pinned slice are not what limits the quality stream either: framed into HBM and brought down by
// the copy engine, the same 0.5 s.
struct Downloader {
  static constexpr size_t SLICE = 64u << 20;
  Stream s;  // (in front of the slices and events: it goes last)
  HBuf pin[2];
  Event ev[2];
  Downloader() {
    HIPOK(s.create());
    for (int i = 0; i < 2; i++) { HIPOK(pin[i].alloc(SLICE)); HIPOK(ev[i].create()); }
  }
  void to_file(scalce_ctx *ctx, scalce_batch *b, int which, int mate, OutFile &f) {
    const void *d = nullptr;
    uint64_t n = 0;
    SCOK(ctx, scalce_batch_output(b, which, mate, &d, &n));
    range_to_file(static_cast<const uint8_t *>(d), n, f);
  }
  // the coded quality stream: framed on its way into the pinned slices (scalce_batch_qual_window), no copy in HBM
  void qual_to_file(scalce_ctx *ctx, scalce_batch *b, int mate, OutFile &f) {
    uint64_t total = 0;
    SCOK(ctx, scalce_batch_qual_bytes(b, mate, &total));
    slices_to_file(total, f, [&](uint8_t *dst, uint64_t off, uint64_t k) { SCOK(ctx, scalce_batch_qual_window(b, mate, off, k, dst, s)); });
  }
  void range_to_file(const uint8_t *src, uint64_t n, OutFile &f) {
    slices_to_file(n, f, [&](uint8_t *dst, uint64_t off, uint64_t k) {
      HIPOK(hipMemcpyAsync(dst, src + off, k, hipMemcpyDeviceToHost, s));
    });
  }
  // n bytes in slices: fill(dst, off, k) enqueues bytes off .. off + k of the stream into pinned slice dst on s
  template <class Fill> void slices_to_file(uint64_t n, OutFile &f, Fill fill) {
    const uint64_t nslices = (n + SLICE - 1) / SLICE;
    auto start = [&](uint64_t i) {
      const uint64_t off = i * SLICE;
      fill(pin[i & 1].as<uint8_t>(), off, std::min<uint64_t>(SLICE, n - off));
      HIPOK(hipEventRecord(ev[i & 1], s));
    };
    if (nslices) start(0);
    for (uint64_t i = 0; i < nslices; i++) {
      HIPOK(hipEventSynchronize(ev[i & 1]));
      if (i + 1 < nslices) start(i + 1);
      f.write(pin[i & 1].as<uint8_t>(), (size_t)std::min<uint64_t>(SLICE, n - i * SLICE));
    }
  }
};

// ---- run setup --------------------------------------------------------------------------------------------
static scalce_params params_from(const Options &o) {
  scalce_params p;
  scalce_params_default(&p);
  p.paired = o.pairs(); p.use_names = o.use_names; p.no_ac = o.no_ac; p.bucket_set_size = o.bucket_set_size;
  p.fasta = o.fasta; p.no_qualities = o.no_qual; p.interleaved = o.interleave;
  p.variable_length = o.varlen;
  return p;
}
// the same for -d; lens[m]: mate m's length stream, open where has_lens[m] says the archive has one
static scalce_unpack_params unpack_params_from(const Options &o, int nm, ArchiveFile lens[2], const bool has_lens[2]) {
  scalce_unpack_params p;
  memset(&p, 0, sizeof p);
  for (int m = 0; m < nm; m++) {
    if (!has_lens[m]) continue;
    p.len_rd[m] = ArchiveFile::read;
    p.len_user[m] = &lens[m];
    p.len_skip[m] = lens[m].gz ? nullptr : ArchiveFile::skip;
  }
  p.mates = nm;
  p.interleave = o.interleave;
  p.no_qualities = o.fasta || o.no_qual;  // -d -Q / -d -f: two-line records, whatever the .scalceq holds (decompress.cpp:159-168)
  p.mate_digit = o.pairs();
  p.ignore_names = !o.use_names;          // decompress.cpp:219-237
  p.library = o.library.c_str();
  p.split = o.split;
  p.window_text_bytes = o.window;
  return p;
}
// --records (the whole archive without it); a plain file of the archive can be passed over by seeking
static scalce_unpack_range unpack_range_from(const Options &o, int nm, ArchiveFile files[2][3]) {
  scalce_unpack_range rg;
  memset(&rg, 0, sizeof rg);
  rg.first_record = o.range_first;
  rg.nrecords = o.range_count;
  for (int m = 0; m < nm; m++)
    for (int k = 0; k < 3; k++) rg.skip[m][k] = files[m][k].gz ? nullptr : ArchiveFile::skip;
  return rg;
}
// Mate m's quality map and read length from the first records of the first input file (get_quality_stats,
// compress.cpp:761).  fill_peek holds at the end of that file; under --gpus, where several files were written out as one,
// the sample ends where the first file did (first_file_bytes).  -f: the statistics stay zero, so the offset stays 64
// (qualities.cpp:91-101); -Q samples as usual: the offset in the header is the one detected.
// -i: both mates from the one source, every other record of it (mate m's first record is record m).
static void quality_model(const Options &o, MateSource &src, int m, scalce_params &p, bool log) {
  const int stride = o.interleave ? 2 : 1, first = o.interleave ? m : 0;
  src.fill_peek(stride * (o.fasta ? 1 : o.sample), o.fasta ? 2 : 4);
  const size_t n = o.first_file_bytes[m] ? std::min<size_t>(src.peek.size(), o.first_file_bytes[m]) : src.peek.size();
  int32_t qhist[128] = {0};
  int rl = 0;
  if (o.fasta) {  // nothing is sampled (qualities.cpp:65): the read length is that of line 2 of the (mate's) first record
    const uint8_t *t = src.peek.data(), *e = t + n, *nl = nullptr;
    for (int k = 0; k < 2 * first + 1 && t < e; k++, t = nl + 1)  // behind the name line of record `first`
      if (!(nl = (const uint8_t *)memchr(t, '\n', (size_t)(e - t)))) break;
    const uint8_t *nl2 = nl && nl + 1 < e ? (const uint8_t *)memchr(nl + 1, '\n', (size_t)(e - (nl + 1))) : nullptr;
    if (nl2) rl = (int)(nl2 - nl - 1);
  } else if (o.varlen) {  // the longest sampled read (or --max-length); the histogram counts the characters that are there
    int32_t longest = 0;
    scalce_varlen_sample(src.peek.data(), n, o.sample, stride, first, o.max_length, qhist, &longest);
    rl = longest;
  } else {
    sample_stats(src.peek.data(), n, o.sample, qhist, rl, stride, first);
  }
  scalce_qmap_init(&p.qmap[m], qhist, o.lossy);
  p.read_len[m] = rl;
  if (log) LOG("\tPaired end #%d, quality offset: %d\n\t               read length: %d\n", m + 1, p.qmap[m].offset, rl);
}
// The device context with the core table loaded: -P LIST, --patterns-bin FILE, $SCALCE_PATTERNS or patterns.bin next to
// the executable.  The table's bytes come back in `table`.  --gpus forks before anything touches HIP: this runs in main()
// on one GPU and inside each rank, never in the parent of a --gpus run.
static scalce_ctx *open_device(const Options &o, const char *argv0, int device, std::vector<uint8_t> &table, bool &is_text) {
  scalce_ctx *ctx = nullptr;
  if (scalce_ctx_create(device, &ctx)) FAIL("%s\n", scalce_last_error(ctx));
  is_text = !o.patterns.empty();
  if (is_text) table = read_whole(o.patterns);
  else {
    std::vector<std::string> cand;
    if (!o.patterns_bin.empty()) cand.push_back(o.patterns_bin);
    if (const char *e = getenv("SCALCE_PATTERNS")) cand.push_back(e);
    const size_t sl = std::string(argv0).rfind('/');
    cand.push_back((sl == std::string::npos ? std::string(".") : std::string(argv0, sl)) + "/patterns.bin");
    cand.push_back("patterns.bin");
    auto found = std::find_if(cand.begin(), cand.end(), [](const std::string &c) { struct stat st; return stat(c.c_str(), &st) == 0; });
    if (found == cand.end())
      FAIL("No core table: give --patterns-bin FILE, -P LIST or set SCALCE_PATTERNS (the reference embeds patterns.bin at link time)\n");
    table = read_whole(*found);
  }
  if (is_text) SCOK(ctx, scalce_patterns_load_text(ctx, (const char *)table.data(), table.size()));
  else SCOK(ctx, scalce_patterns_load_bin(ctx, table.data(), table.size()));
  return ctx;
}
// the statistics lines both compress paths print
static void log_statistics(const Options &o, const scalce_params &p, uint64_t N, uint64_t unbucketed) {
  LOG("Statistics:\n\tTotal number of reads: %llu\n\tRead length: first end %d\n", (unsigned long long)N, p.read_len[0]);
  if (o.pairs()) LOG("\t             second end %d\n", p.read_len[1]);
  LOG("\tUnbucketed reads count: %llu, bucketed percentage %.2lf\n", (unsigned long long)unbucketed,
      N ? 100.0 * (double)(N - unbucketed) / (double)N : 0.0);
  LOG("\tLossy percentage: %d\n", o.lossy);
}

// ---- compress -----------------------------------------------------------------------------------------
// A mate's files of the archive, out of the batch of a finished run.  One thread per mate calls these.
struct MateFiles {
  const Options &o;
  const scalce_params &p;
  scalce_ctx *ctx;
  scalce_batch *b;
  void write_reads_and_names(int m, Downloader &down) const {
    OutFile fR, fN;
    fR.open(archive_path(o.out, m, 'r'), gz_container(o, 'r'));
    fR.write(reads_header(o, p.read_len[m]));
    down.to_file(ctx, b, SCALCE_OUT_READS, m, fR);
    fR.close();
    fN.open(archive_path(o.out, m, 'n'), gz_container(o, 'n'));
    fN.write(names_header(o));
    if (o.use_names) down.to_file(ctx, b, SCALCE_OUT_NAMES, 0, fN);  // mate 2 repeats mate 1's names (:450-454)
    fN.close();
  }
  void write_lengths(int m) const {  // --variable-length: how long each record really was, in archive order
    OutFile fL;
    fL.open(archive_path(o.out, m, 'l'), gz_container(o, 'l'));
    side_file_header<scalce_host::LEN_HEADER_BYTES>(fL, scalce_host::len_header_write, p.read_len[m]);
    const std::vector<uint8_t> pad = fetch(ctx, b, SCALCE_OUT_LENGTHS, m);
    const int width = scalce_host::len_entry_width(p.read_len[m]);
    std::vector<uint8_t> entries(pad.size() / 2 * (size_t)width);
    scalce_host::len_entries_write(reinterpret_cast<const uint16_t *>(pad.data()), pad.size() / 2, width, entries.data());
    fL.write(entries);
    fL.close();
  }
  void write_order() const {  // --keep-order: the input index of every record (pair), in archive order
    OutFile fO;
    fO.open(archive_path(o.out, 0, 'o'), gz_container(o, 'o'));
    const std::vector<uint8_t> perm = fetch(ctx, b, SCALCE_OUT_PERM, 0);
    side_file_header<scalce_host::ORDER_HEADER_BYTES>(fO, scalce_host::order_header_write, perm.size() / 4);
    fO.write(perm);
    fO.close();
  }
  void write_comments(int m, Downloader &down, uint64_t N) const {  // --keep-comments: what follows each name, in archive order
    OutFile fC;
    fC.open(archive_path(o.out, m, 'c'), gz_container(o, 'c'));
    uint64_t nbytes = 0;
    uint32_t longest = 0;
    SCOK(ctx, scalce_batch_comments_info(b, m, &nbytes, &longest));
    side_file_header<scalce_host::COMMENT_HEADER_BYTES>(fC, scalce_host::comment_header_write, longest, N);
    down.to_file(ctx, b, SCALCE_OUT_COMMENTS, m, fC);
    fC.close();
  }
  void write_plus(int m, Downloader &down, uint64_t N) const {  // --keep-plus: the '+' lines as entries, in archive order
    OutFile fP;
    fP.open(archive_path(o.out, m, 'p'), gz_container(o, 'p'));
    uint32_t longest = 0;
    SCOK(ctx, scalce_batch_plus_info(b, m, nullptr, &longest, nullptr, nullptr));
    side_file_header<scalce_host::PLUS_HEADER_BYTES>(fP, scalce_host::plus_header_write, longest, N);
    if (longest) down.to_file(ctx, b, SCALCE_OUT_PLUS, m, fP);  // (P = 0: every line was bare, the file is its header)
    fP.close();
  }
  void write_exceptions(int m, Downloader &down, uint64_t N) const {  // --keep-bases: what the archive does not keep, in archive order
    OutFile fX;
    fX.open(archive_path(o.out, m, 'x'), gz_container(o, 'x'));
    uint64_t entries = 0;
    SCOK(ctx, scalce_batch_exceptions_info(b, m, &entries, nullptr));
    side_file_header<scalce_host::EXCEPTION_HEADER_BYTES>(fX, scalce_host::exception_header_write, (uint32_t)p.read_len[m], N, entries);
    down.to_file(ctx, b, SCALCE_OUT_EXCEPTIONS, m, fX);
    fX.close();
  }
  void write_qualities(int m, Downloader &down, uint64_t N) const {  // once the coder is through; N: records of the run
    OutFile fQ;
    fQ.open(archive_path(o.out, m, 'q'), gz_container(o, 'q'));
    fQ.write(qual_header(p.qmap[0].offset));
    if (!(o.fasta || o.no_qual)) {  // (-Q / -f: the header and nothing else -- no table (:296), no coder blocks (ac_write of nothing))
      if (!o.no_ac) {
        fQ.write(fetch(ctx, b, SCALCE_OUT_TABLE, m));
        const uint64_t total = N * (uint64_t)p.read_len[m];
        fQ.write(&total, 8);
      }
      down.qual_to_file(ctx, b, m, fQ);
    }
    fQ.close();
  }
};

// The input of a one-GPU run: a source per input stream (-i reads both mates from one), with the quality model sampled.
struct CompressInput {
  int nsrc;
  MateSource src[2];
  uint64_t original = 0, bytes1 = 0;  // input bytes: every mate's, mate 1's
  bool plain1 = true;                 // no gzip among mate 1's files
  CompressInput(const Options &o, const std::vector<std::string> &files, scalce_params &p) : nsrc(o.paired ? 2 : 1) {
    if (o.interleave) src[0].pair_lines = 2 * (o.fasta ? 2 : 4);
    for (int m = 0; m < nsrc; m++) {
      for (const std::string &f : files) {
        const std::string path = mate_file(f, m);
        struct stat st;
        const uint64_t size = stat(path.c_str(), &st) == 0 ? (uint64_t)st.st_size : 0;
        original += size;
        if (m == 0) { bytes1 += size; plain1 = plain1 && !is_gzip(path); }
        src[m].files.push_back(path);
      }
      quality_model(o, src[m], m, p, true);
    }
    if (o.interleave) quality_model(o, src[0], 1, p, true);
    if (p.read_len[0] <= 0) FAIL("Cannot determine the read length of %s\n", files[0].c_str());
  }
  // rows to expect: exact enough for plain text (a record is 2 L + 6 bytes plus its name), unknown behind gzip
  uint64_t rows_hint(const Options &o, const scalce_params &p) const {
    return plain1 ? bytes1 / ((o.fasta ? 1 : 2) * (uint64_t)p.read_len[0] + (o.fasta ? 4 : 8)) / (o.interleave ? 2 : 1) + 64 : 0;
  }
  uint64_t piece_bytes(uint64_t hint) const {
    uint64_t piece = 256ull << 20;  // per chunk; three of them are pinned per mate
    if (const char *e = getenv("SCALCE_PIECE_BYTES")) piece = strtoull(e, nullptr, 10);
    if (hint && bytes1 + (1u << 20) < piece) piece = bytes1 + (1u << 20);  // small inputs: no point in pinning gigabytes
    return piece;
  }
};

static int do_compress(const Options &o, const std::vector<std::string> &files, scalce_ctx *ctx) {
  const double t0 = now();
  const int nm = o.pairs() ? 2 : 1;
  scalce_params p = params_from(o);
  LOG("Preprocessing FASTQ files ...\n");
  CompressInput in(o, files, p);
  const int nsrc = in.nsrc;
  const uint64_t hint = in.rows_hint(o, p), piece = in.piece_bytes(hint);
  scalce_batch *b = nullptr;
  scalce_stream_stats ss;
  char emsg[512] = "";
  const double t1 = now();
  if (scalce_stream_compress(ctx, &p, MateSource::read_cb, &in.src[0], nsrc == 2 ? MateSource::read_cb : nullptr, nsrc == 2 ? &in.src[1] : nullptr,
                             piece, hint, SCALCE_STREAM_LEAN | SCALCE_STREAM_DEFER_ENTROPY | (o.keep_order ? SCALCE_STREAM_KEEP_ORDER : 0) |
                                 (o.keep_comments ? SCALCE_STREAM_KEEP_COMMENTS : 0) | (o.keep_bases ? SCALCE_STREAM_KEEP_BASES : 0) |
                                 (o.keep_plus ? SCALCE_STREAM_KEEP_PLUS : 0) | (o.digest ? SCALCE_STREAM_DIGEST : 0), &b, &ss, emsg, sizeof emsg)) {
    if (!in.src[0].error.empty()) fputs(in.src[0].error.c_str(), stderr);  // (-i: a file of odd record count; the stream only saw a read error)
    else fprintf(stderr, "%s\n", emsg[0] ? emsg : scalce_last_error(ctx));
    exit(1);
  }
  const double t2 = now();
  const uint64_t N = scalce_batch_reads(b);
  LOG("\tDone with file %s, %llu reads found\n", files[0].c_str(), (unsigned long long)N);
  uint32_t st4[7] = {0, 0, 0, 0, 0, 0, 0};
  scalce_batch_stats(b, st4);
  // the arithmetic coder starts on its own stream; the read and name streams come down and are written beside it
  // (a run of up to 2048 blocks is one launch that takes as long as ONE block's serial chain, about 0.3 s)
  Stream s_ent;
  HIPOK(s_ent.create());
  SCOK(ctx, scalce_batch_set_frame_on_demand(b, 1));  // the coded blocks are framed on their way into the pinned slices
  SCOK(ctx, scalce_batch_entropy_begin(b, nullptr, s_ent));

  // the files of a mate are written by a thread of its own (paired runs: two mates, two sets of files, two threads)
  auto per_mate = [&](auto &&body) {
    if (nm == 1) { body(0); return; }
    std::vector<std::thread> ts;
    for (int m = 0; m < nm; m++) ts.emplace_back([&body, m]() { HIPOK(hipSetDevice(0)); body(m); });
    for (auto &t : ts) t.join();
  };
  std::unique_ptr<Downloader> downs[2];  // (a mate's pinned slices serve both of its passes)
  const MateFiles w{o, p, ctx, b};
  per_mate([&](int m) {
    downs[m].reset(new Downloader);
    w.write_reads_and_names(m, *downs[m]);
    if (o.varlen) w.write_lengths(m);
    if (o.keep_order && m == 0) w.write_order();
    if (o.keep_comments) w.write_comments(m, *downs[m], N);
    if (o.keep_bases) w.write_exceptions(m, *downs[m], N);
    if (o.keep_plus) w.write_plus(m, *downs[m], N);
  });
  // (an order stream left under this prefix by an earlier run does not belong to this archive, nor do comment streams)
  if (!o.keep_order) unlink(archive_path(o.out, 0, 'o').c_str());
  if (!o.keep_comments) for_each_archive_file(o, "c", [](char, const std::string &fn) { unlink(fn.c_str()); });
  if (!o.keep_bases) for_each_archive_file(o, "x", [](char, const std::string &fn) { unlink(fn.c_str()); });
  if (!o.keep_plus) for_each_archive_file(o, "p", [](char, const std::string &fn) { unlink(fn.c_str()); });
  // --digest: what the run read, one entry per mate stream (a digest stream left by an earlier run goes like the others)
  scalce_host::Digest dg;
  if (o.digest) {
    dg.kind = (o.paired ? scalce_host::DIGEST_KIND_PAIRED : o.interleave ? scalce_host::DIGEST_KIND_INTERLEAVED : scalce_host::DIGEST_KIND_SINGLE) |
              (o.fasta ? scalce_host::DIGEST_KIND_FASTA : 0);
    dg.texts = nsrc;
    for (int m = 0; m < nsrc; m++) { dg.text[m].bytes = ss.bytes[m]; dg.text[m].crc = ss.crc[m]; }
    uint8_t raw[scalce_host::DIGEST_MAX_BYTES];
    const size_t n = scalce_host::digest_write(raw, dg);
    OutFile fD;
    fD.open(archive_path(o.out, 0, 'd'), gz_container(o, 'd'));
    fD.write(raw, n);
    fD.close();
  } else {
    unlink(archive_path(o.out, 0, 'd').c_str());
  }
  const double t2b = now();
  SCOK(ctx, scalce_batch_finish(b, s_ent));  // the coder is through: sizes of the coded streams, device error word
  const double t2c = now();
  per_mate([&](int m) {
    w.write_qualities(m, *downs[m], N);
    downs[m].reset();
  });
  const double t2d = now();
  uint64_t new_size = 0;
  const std::string exts = std::string("rnql") + (o.keep_order ? "o" : "") + (o.keep_comments ? "c" : "") + (o.keep_bases ? "x" : "") + (o.keep_plus ? "p" : "");
  for_each_archive_file(o, exts.c_str(), [&](char, const std::string &fn) {
    struct stat st;
    if (stat(fn.c_str(), &st) == 0) new_size += (uint64_t)st.st_size;
  });
  s_ent.release();
  const void *dc = nullptr;
  uint64_t nc = 0;
  SCOK(ctx, scalce_batch_output(b, SCALCE_OUT_BUCKET_COUNTS, 0, &dc, &nc));
  uint64_t unbucketed = 0;
  if (nc >= 8) SCOK(ctx, scalce_memcpy_d2h(ctx, &unbucketed, (const uint8_t *)dc + nc - 8, 8));
  uint64_t com_bytes[2] = {0, 0};
  uint32_t com_longest[2] = {0, 0};
  for (int m = 0; m < nm && o.keep_comments; m++) SCOK(ctx, scalce_batch_comments_info(b, m, &com_bytes[m], &com_longest[m]));
  uint64_t exc_entries[2] = {0, 0}, exc_rows[2] = {0, 0};
  for (int m = 0; m < nm && o.keep_bases; m++) SCOK(ctx, scalce_batch_exceptions_info(b, m, &exc_entries[m], &exc_rows[m]));
  uint32_t plus_longest[2] = {0, 0};
  uint64_t plus_rep[2] = {0, 0}, plus_lit[2] = {0, 0};
  for (int m = 0; m < nm && o.keep_plus; m++) SCOK(ctx, scalce_batch_plus_info(b, m, nullptr, &plus_longest[m], &plus_rep[m], &plus_lit[m]));
  scalce_batch_destroy(b);
  const double t3 = now();
  log_statistics(o, p, N, unbucketed);
  for (int m = 0; m < nm && o.keep_bases; m++) exception_log(N, exc_entries[m], exc_rows[m]);
  for (int m = 0; m < nm && o.keep_comments; m++) comment_log(N, com_bytes[m], com_longest[m]);
  for (int m = 0; m < nm && o.keep_plus; m++) plus_log(N, plus_rep[m], plus_lit[m], plus_longest[m]);
  for (int m = 0; m < dg.texts; m++) LOG("\tDigest: %llu bytes, crc32 %08x\n", (unsigned long long)dg.text[m].bytes, dg.text[m].crc);
  LOG("\tSpill chunks: %u, pieces streamed: %llu\n", st4[3], (unsigned long long)ss.rounds);
  LOG("\tTime elapsed: %.2f s (sample %.2f; stream %.2f = waiting for the reader %.2f + for uploads %.2f + ingest/count/tokenize %.2f; "
      "order %.2f, emit %.2f; reads+names down and written beside the coder %.2f, waiting for the coder %.2f, qualities down and written %.2f, device buffers released %.2f)\n",
      t3 - t0, t1 - t0, ss.total_s - ss.order_s - ss.emit_s, ss.read_wait_s, ss.h2d_wait_s, ss.front_s, ss.order_s, ss.emit_s,
      t2b - t2, t2c - t2b, t2d - t2c, t3 - t2d);
  LOG("\tOriginal size: %.2lfM, new size: %.2lfM, compression factor: %.2lf\n", in.original / (1024.0 * 1024.0),
      new_size / (1024.0 * 1024.0), new_size ? (double)in.original / (double)new_size : 0.0);
  return 0;
}

// ---- compress on several GPUs ---------------------------------------------------------------------------------
// One process per GPU (forked before anything touches a GPU), rank r takes the r-th part of the input file, the ranks talk
// RCCL (scalce_sharded_compress) and every rank writes its pieces of the ONE archive with pwrite at the offsets the
// run-wide bucket counts give.  SCALCE_COMM=shm makes all ranks share GPU 0 over the shared-memory rehearsal transport.
// A rank's steps, in the order rank_main() takes them.

// 1. The communicator: the shared-memory transport, or RCCL with the id rank 0 publishes in a file next to the output.
static scalce_comm *open_comm(const Options &o, bool shm, int device, int world, int rank, const std::string &tag) {
  scalce_comm *comm = nullptr;
  if (shm) {
    if (scalce_comm_create_shm(device, world, rank, ("/scalce_cli_" + tag).c_str(), 1ull << 30, &comm)) FAIL("%s\n", scalce_comm_error(comm));
    return comm;
  }
  const std::string idfile = o.out + ".rcclid." + tag;
  uint8_t id[SCALCE_COMM_ID_BYTES];
  if (rank == 0) {
    if (scalce_comm_unique_id(id)) FAIL("RCCL is not available\n");
    FILE *f = fopen((idfile + ".tmp").c_str(), "wb");
    if (!f || fwrite(id, 1, sizeof id, f) != sizeof id) FAIL("Cannot write %s\n", idfile.c_str());
    fclose(f);
    rename((idfile + ".tmp").c_str(), idfile.c_str());
  } else {
    FILE *f = nullptr;
    for (int tries = 0; tries < 60000 && !(f = fopen(idfile.c_str(), "rb")); tries++) usleep(1000);
    if (!f || fread(id, 1, sizeof id, f) != sizeof id) FAIL("rank 0 did not publish the RCCL id\n");
    fclose(f);
  }
  if (scalce_comm_create_rccl(device, world, rank, id, &comm)) FAIL("%s\n", scalce_comm_error(comm));
  scalce_comm_barrier(comm, nullptr);
  if (rank == 0) unlink(idfile.c_str());
  return comm;
}

// one mate's input file as a rank holds it, and the bytes [lo, hi) of it that are the rank's records
struct RankInput {
  std::string path;
  Fd fd;
  uint64_t size = 0, lo = 0, hi = 0;
};
// 2. The quality model: the first records of the FILE, the same on every rank (get_quality_stats, compress.cpp:761).
static void open_rank_inputs(const Options &o, const std::vector<std::string> &files, int nm, bool log, scalce_params &p, RankInput in[2]) {
  in[0].path = files[0];
  in[1].path = mate_file(files[0], o.paired ? 1 : 0);
  for (int m = 0; m < nm; m++) {
    if (is_gzip(in[m].path)) FAIL("--gpus needs plain (not gzip) input: the file is split by byte ranges\n");
    MateSource src;
    src.files.push_back(in[m].path);
    quality_model(o, src, m, p, log);
    struct stat st;
    if (!in[m].fd.open(in[m].path, O_RDONLY) || fstat(in[m].fd.get(), &st) != 0) FAIL("Cannot read file %s\n", in[m].path.c_str());
    in[m].size = (uint64_t)st.st_size;
  }
  if (p.read_len[0] <= 0) FAIL("Cannot determine the read length of %s\n", files[0].c_str());
}
// 3. This rank's records of mate m: a line-aligned byte range, the line counts of everybody (one all-gather through the
// 64 + 64 * 4 words of d_io), then cuts at multiples of four lines (cli_shares.hpp).  K: where every rank's records begin,
// made from mate 1 and kept for mate 2.
static void record_range(scalce_comm *comm, hipStream_t s, uint64_t *d_io, int rank, int world, int m, RankInput &in, std::vector<uint64_t> &K) {
  const int fd = in.fd.get();
  const uint64_t a = line_start(fd, in.size, world, rank), b = line_start(fd, in.size, world, rank + 1);
  uint64_t mine[2] = {count_newlines(fd, a, b, std::max(1, std::min(g_threads, 16))), a};
  std::vector<uint64_t> all((size_t)world * 2);
  HIPOK(hipMemcpy(d_io, mine, sizeof mine, hipMemcpyHostToDevice));
  if (scalce_comm_all_gather(comm, d_io, d_io + 64, sizeof mine, s)) FAIL("%s\n", scalce_comm_error(comm));
  HIPOK(hipStreamSynchronize(s));
  HIPOK(hipMemcpy(all.data(), d_io + 64, all.size() * 8, hipMemcpyDeviceToHost));
  const LineRanges ranges(world, all.data());
  switch (ranges.refusal(m ? &K : nullptr)) {
    case LineRanges::NOT_WHOLE_RECORDS: FAIL("%s has %llu lines: not a multiple of 4\n", in.path.c_str(), (unsigned long long)ranges.lines());
    case LineRanges::MATES_DIFFER: FAIL("mates have different record counts\n");
    case LineRanges::OK: break;
  }
  if (m == 0) K = ranges.first_records();
  in.lo = ranges.offset_of_line(fd, in.size, 4 * K[rank]);
  in.hi = ranges.offset_of_line(fd, in.size, 4 * K[rank + 1]);
}
// 4. The piece into HBM, through two pinned chunks in turn.
static void upload_piece(RankInput in[2], int nm, hipStream_t s, DBuf d_text[2]) {
  const size_t CH = 256u << 20;
  HBuf pin_buf[2];  // (both go at the end of this function, behind the stream's synchronisation)
  Event ev[2];
  uint8_t *pin[2];
  for (int i = 0; i < 2; i++) { HIPOK(pin_buf[i].alloc(CH)); HIPOK(ev[i].create()); pin[i] = pin_buf[i].as<uint8_t>(); }
  for (int m = 0; m < nm; m++) {
    const uint64_t n = in[m].hi - in[m].lo;
    HIPOK(dbuf_alloc(d_text[m], n + 256));
    uint64_t done = 0;
    for (int i = 0; done < n; i ^= 1) {
      HIPOK(hipEventSynchronize(ev[i]));
      const uint64_t k = std::min<uint64_t>(CH, n - done);
      if (!pread_parallel(in[m].fd.get(), pin[i], k, in[m].lo + done, 16u << 20, g_threads_io())) FAIL("Read error\n");
      HIPOK(hipMemcpyAsync(d_text[m].as<uint8_t>() + done, pin[i], k, hipMemcpyHostToDevice, s));
      HIPOK(hipEventRecord(ev[i], s));
      done += k;
    }
  }
  HIPOK(hipStreamSynchronize(s));
}
// 5. The sharded run over the uploaded pieces; the batch holds this rank's streams, res the run-wide counts.
static scalce_batch *run_sharded(scalce_comm *comm, scalce_ctx *ctx, const scalce_params &p, const RankInput in[2], int nm, DBuf d_text[2],
                                 hipStream_t s, scalce_shard_result &res) {
  scalce_batch *b = nullptr;
  const uint64_t n0 = in[0].hi - in[0].lo, n1 = nm == 2 ? in[1].hi - in[1].lo : 0;
  const uint64_t rows = n0 / (2 * (uint64_t)p.read_len[0] + 7) + 64;
  SCOK(ctx, scalce_batch_create(ctx, &p, rows + rows / 3, std::max(n0, n1) + 256, &b));
  memset(&res, 0, sizeof res);
  if (scalce_sharded_compress(comm, ctx, b, d_text[0].as<uint8_t>(), n0, nm == 2 ? d_text[1].as<uint8_t>() : nullptr, n1, 0, s, nullptr, &res))
    exit(1);
  for (int m = 0; m < nm; m++) d_text[m].release();
  return b;
}
// 6. Every rank writes its pieces of the archive: per file, rank 0 (`lead`) creates it and writes the header, everybody
// opens it behind a barrier and places its share.
struct ShareWriter {
  const Options &o;
  const scalce_params &p;
  scalce_ctx *ctx;
  scalce_batch *b;
  scalce_comm *comm;
  hipStream_t s;
  const int rank;
  const bool lead;
  const scalce_shard_result &res;
  const Shares reads, names;  // records and name bytes per mate-1 bucket
  std::vector<int32_t> bucket_pattern;
  std::vector<uint64_t> recsz;  // bytes of a mate-1 record per bucket: the bases its core does not give, and the metadata
  ShareWriter(const Options &o_, const scalce_params &p_, scalce_ctx *ctx_, scalce_batch *b_, scalce_comm *comm_, hipStream_t s_, int rank_, int world,
              const scalce_shard_result &res_, const std::vector<uint8_t> &table, bool is_text)
      : o(o_), p(p_), ctx(ctx_), b(b_), comm(comm_), s(s_), rank(rank_), lead(rank_ == 0), res(res_), reads(res_.counts, res_.nb1, world, rank_),
        names(res_.name_bytes, res_.nb1, world, rank_), bucket_pattern(res_.nb1), recsz(res_.nb1) {
    int32_t nst = 0, nbk = 0;
    scalce_patterns_describe_host(table.data(), table.size(), is_text ? 1 : 0, bucket_pattern.data(), res.nb1, &nst, &nbk);
    const int L0 = p.read_len[0], sz_meta = L0 > 255 ? 2 : 1;
    for (uint32_t k = 0; k < res.nb1; k++) {
      const int lv = bucket_pattern[k] == SCALCE_ROOT_CORE ? 0 : scalce_pattern_length(ctx, bucket_pattern[k]);
      recsz[k] = (uint64_t)((L0 - lv + 3) / 4 + sz_meta);
    }
  }
  Fd open_out(int m, char ext, const std::vector<uint8_t> &header) const {
    const std::string fn = archive_path(o.out, m, ext);
    Fd f;
    if (lead && !f.open(fn, O_CREAT | O_TRUNC | O_WRONLY, 0644)) FAIL("Cannot create %s\n", fn.c_str());
    f.release();
    scalce_comm_barrier(comm, s);
    if (!f.open(fn, O_WRONLY)) FAIL("Cannot open %s\n", fn.c_str());
    if (lead) pwrite_all(f.get(), header.data(), header.size(), 0);
    return f;
  }
  void write_reads(int m) const {  // .scalcer: mate 1 in buckets, mate 2 bare rows in mate 1's order
    const uint64_t w = ((uint64_t)p.read_len[m] + 3) / 4;
    const std::vector<uint8_t> h = reads_header(o, p.read_len[m]), mine = fetch(ctx, b, SCALCE_OUT_READS, m);
    const Fd f = open_out(m, 'r', h);
    if (m == 0) place_share(f.get(), h.size(), mine.data(), reads, [&](size_t k) { return recsz[k]; }, bucket_pattern.data(), lead);
    else place_share(f.get(), h.size(), mine.data(), reads, [w](size_t) { return w; });
  }
  void write_names(int m) const {  // .scalcen (mate 2 repeats mate 1's names, compress.cpp:450-454)
    const std::vector<uint8_t> h = names_header(o);
    const Fd f = open_out(m, 'n', h);
    if (o.use_names) place_share(f.get(), h.size(), fetch(ctx, b, SCALCE_OUT_NAMES, 0).data(), names, [](size_t) { return (uint64_t)1; });
  }
  void write_qualities(int m) const {  // .scalceq
    const uint64_t L = (uint64_t)p.read_len[m];
    const std::vector<uint8_t> h = qual_header(p.qmap[0].offset);
    const Fd f = open_out(m, 'q', h);
    if (!o.no_ac) {  // the table and the symbol count, then the coded blocks of every rank in rank order
      if (lead) {
        const std::vector<uint8_t> tb = fetch(ctx, b, SCALCE_OUT_TABLE, m);
        pwrite_all(f.get(), tb.data(), tb.size(), h.size());
        const uint64_t total = res.reads_total * L;
        pwrite_all(f.get(), &total, 8, h.size() + tb.size());
      }
      uint64_t before = 0;
      for (int r = 0; r < rank; r++) before += res.coded_bytes[m][r];
      const std::vector<uint8_t> mine = fetch(ctx, b, SCALCE_OUT_QUAL, m);
      pwrite_all(f.get(), mine.data(), mine.size(), h.size() + QTABLE_WORDS * 4 + 8 + before);
    } else {  // -A: the raw q' rows, bucket by bucket in rank order (compress.cpp:389-390)
      place_share(f.get(), h.size(), fetch(ctx, b, SCALCE_OUT_QSTREAM, m).data(), reads, [L](size_t) { return L; });
    }
  }
};

static int rank_main(const Options &o, const std::vector<std::string> &files, const char *argv0, int rank, int world, const std::string &tag) {
  const bool shm = getenv("SCALCE_COMM") && !strcmp(getenv("SCALCE_COMM"), "shm");
  const int device = shm ? 0 : rank;
  const int nm = o.paired ? 2 : 1;
  const double t0 = now();
  std::vector<uint8_t> table;
  bool is_text = false;
  scalce_ctx *ctx = open_device(o, argv0, device, table, is_text);
  scalce_comm *comm = open_comm(o, shm, device, world, rank, tag);
  scalce_params p = params_from(o);
  RankInput in[2];
  open_rank_inputs(o, files, nm, rank == 0, p, in);
  Stream s;
  HIPOK(s.create());
  DBuf d_io;
  HIPOK(dbuf_alloc(d_io, sizeof(uint64_t) * (64 + 64 * 4)));
  std::vector<uint64_t> K;  // rank r starts at record K[r], in every mate
  for (int m = 0; m < nm; m++) record_range(comm, s, d_io.as<uint64_t>(), rank, world, m, in[m], K);
  DBuf d_text[2];
  upload_piece(in, nm, s, d_text);
  const double t1 = now();
  scalce_shard_result res;
  scalce_batch *b = run_sharded(comm, ctx, p, in, nm, d_text, s, res);
  const double t2 = now();
  const ShareWriter w(o, p, ctx, b, comm, s, rank, world, res, table, is_text);
  for (int m = 0; m < nm; m++) {
    w.write_reads(m);
    w.write_names(m);
    w.write_qualities(m);
  }
  scalce_comm_barrier(comm, s);
  const double t3 = now();
  if (w.lead) {
    LOG("\tDone with file %s, %llu reads found\n", files[0].c_str(), (unsigned long long)res.reads_total);
    log_statistics(o, p, res.reads_total, w.reads.all[res.nb1 - 1]);
    LOG("\tGPUs: %d, spill chunks: %u, tie-break rounds: %u\n", world, res.chunks_total, res.rounds);
    LOG("\tTime elapsed: %.2f s (split + read + upload %.2f, sharded hot path %.2f, download + write %.2f)\n", t3 - t0, t1 - t0, t2 - t1, t3 - t2);
  }
  scalce_shard_result_free(&res);
  scalce_batch_destroy(b);
  scalce_comm_destroy(comm);
  scalce_ctx_destroy(ctx);
  return 0;
}

// --gpus splits ONE plain file per mate by byte ranges.  Several input files, or gzip input (the reference runs any number
// of files, each through its gz reader, compress.cpp:756-811): the record stream of every mate -- the files one after the
// other, inflated -- is written out once as a plain file under -t, and the ranks split that.
static bool plain_single_input(const Options &o, const std::vector<std::string> &files) {
  if (files.size() != 1) return false;
  for (int m = 0; m < (o.paired ? 2 : 1); m++) {
    std::string path = files[0];
    if (m && !second_file(files[0], path)) return true;  // (the rank reports it)
    if (is_gzip(path)) return false;
  }
  return true;
}
// files the parent of a --gpus run must not leave behind, whichever way it ends (FAIL() is exit(1): atexit runs; the ranks
// leave through _exit and never get here)
static std::vector<std::string> g_unlink_at_exit;
static void unlink_at_exit() { for (auto &f : g_unlink_at_exit) unlink(f.c_str()); }
static std::string materialize_inputs(Options &o, const std::vector<std::string> &files, const std::string &tag) {
  struct stat st;
  std::string dir = o.temp;
  // (no silent fall-back to /tmp: at full size this is 100+ GB, and the user said where temporary files go)
  if (stat(dir.c_str(), &st) != 0 && mkdir(dir.c_str(), 0777) != 0) FAIL("Cannot create temporary directory %s (-t)\n", dir.c_str());
  atexit(unlink_at_exit);
  // the mate digit is the LAST '1' of the path (get_second_file, const.cpp:51-64): it closes the name
  std::string base = dir + "/scalce_gpus_" + tag + "_m";
  for (char &c : base) if (&c >= &base[dir.size()] && c == '1') c = 'x';
  std::vector<uint8_t> buf(64u << 20);
  for (int m = 0; m < (o.paired ? 2 : 1); m++) {
    MateSource src;
    for (auto &f : files) {
      const std::string path = mate_file(f, m);
      if (stat(path.c_str(), &st) != 0) FAIL("File %s does not exist or it is not accessible.\n", path.c_str());
      src.files.push_back(path);
    }
    const std::string out = base + (m ? "2" : "1");
    FILE *f = fopen(out.c_str(), "wb");
    if (!f) FAIL("Cannot create %s\n", out.c_str());
    g_unlink_at_exit.push_back(out);
    uint64_t total = 0;
    for (;;) {
      const size_t before = src.cur;
      const int64_t k = src.read(buf.data(), buf.size());
      if (k < 0) FAIL("Read error\n");
      // (a read never spans two files: the first file has ended when the source has moved on to the second)
      if (!o.first_file_bytes[m] && files.size() > 1 && before >= 1 && src.cur >= 2) o.first_file_bytes[m] = total;
      if (k == 0) break;
      if (fwrite(buf.data(), 1, (size_t)k, f) != (size_t)k) FAIL("write failed (%s)\n", out.c_str());
      total += (uint64_t)k;
    }
    fclose(f);
  }
  return base + "1";
}
// -c gz behind --gpus: the ranks write the plain archive at computed offsets; the streams the reference would have sent
// through its gzip writer are then rewritten as gzip members by this process's threads
static void gzip_in_place(const std::string &path) {
  Fd in;
  if (!in.open(path, O_RDONLY)) FAIL("Cannot read %s\n", path.c_str());
  OutFile out;
  out.open(path + ".gz.tmp", true);
  std::vector<uint8_t> buf(256u << 20);
  for (;;) {
    const ssize_t k = ::read(in.get(), buf.data(), buf.size());
    if (k < 0) FAIL("Read error on %s\n", path.c_str());
    if (k == 0) break;
    out.write(buf.data(), (size_t)k);
  }
  in.release();
  out.close();
  if (rename((path + ".gz.tmp").c_str(), path.c_str()) != 0) FAIL("Cannot replace %s\n", path.c_str());
}

static int multi_gpu_compress(const Options &o_in, const std::vector<std::string> &files_in, const char *argv0) {
  if (o_in.gpus > 64) FAIL("--gpus: at most 64\n");
  LOG("Preprocessing FASTQ files ...\n");
  const std::string tag = std::to_string(getpid()) + "_" + std::to_string((long)time(nullptr));
  set_threads(o_in.threads, 1);
  Options o = o_in;
  o.container = 0;  // the ranks write plain; -c gz is applied to the finished files below
  std::vector<std::string> files = files_in;
  if (!plain_single_input(o, files)) {
    const double t0 = now();
    files.assign(1, materialize_inputs(o, files_in, tag));
    LOG("\t%zu input file(s) per mate written out as one plain file under %s (%.2f s)\n", files_in.size(), o.temp.c_str(), now() - t0);
  }
  set_threads(o.threads, o.gpus);  // (the ranks share the host)
  std::vector<pid_t> kids;
  for (int r = 0; r < o.gpus; r++) {
    const pid_t pid = fork();
    if (pid < 0) FAIL("fork failed\n");
    if (pid == 0) _exit(rank_main(o, files, argv0, r, o.gpus, tag));
    kids.push_back(pid);
  }
  // Ranks are collected in the order they end.  One that fails on its own (a crash, an error outside the collective
  // protocol of scalce_sharded_compress) leaves the others waiting for it in a collective: the first bad exit ends them.
  int bad = 0;
  size_t left = kids.size();
  while (left) {
    int st = 0;
    const pid_t k = waitpid(-1, &st, 0);
    if (k < 0) { if (errno == EINTR) continue; break; }
    auto it = std::find(kids.begin(), kids.end(), k);
    if (it == kids.end()) continue;
    *it = -1;
    left--;
    const bool ok = WIFEXITED(st) && WEXITSTATUS(st) == 0;
    if (!ok && !bad) {
      bad = 1;
      for (pid_t o2 : kids) if (o2 > 0) kill(o2, SIGTERM);
    }
  }
  if (bad) {  // what the ranks had written so far is not an archive: nothing stays behind under the output name
    for_each_archive_file(o, "rnq", [](char, const std::string &fn) { unlink(fn.c_str()); });
    fprintf(stderr, "(ERROR) a rank failed\n");
    return 1;
  }
  if (o_in.container != 0) {
    set_threads(o_in.threads, 1);
    const double t0 = now();
    for_each_archive_file(o, "rnq", [&](char ext, const std::string &fn) { if (gz_container(o_in, ext)) gzip_in_place(fn); });
    LOG("\tgzip containers written by %d host threads: %.2f s\n", g_threads, now() - t0);
  }
  LOG("Done!\n");
  return 0;
}

// ---- decompress ------------------------------------------------------------------------------------------
static std::string scalce_name(std::string path, char c) {  // get_file_name, decompress.cpp:72-77
  size_t p = path.rfind(".scalce");
  if (p != std::string::npos && p + 7 < path.size()) path[p + 7] = c;
  return path;
}
// The archive named by its .scalcen: every mate's three files open behind the read callbacks, and the length streams of a
// variable-length archive.
struct Archive {
  std::string base[2];
  bool has_lens[2] = {false, false};
  bool has_order = false;  // a PREFIX_1.scalceo lies next to the .scalcen (and --archive-order does not set it aside)
  bool has_comments = false;  // every mate has a PREFIX_<m>.scalcec next to its .scalcen (and neither --no-comments nor -n sets them aside)
  ArchiveFile comments[2];
  bool has_exceptions = false;  // every mate has a PREFIX_<m>.scalcex next to its .scalcen (and --stored-bases does not set them aside)
  ArchiveFile exceptions[2];
  bool has_plus = false;  // every mate has a PREFIX_<m>.scalcep next to its .scalcen (and neither --bare-plus nor -Q / -f sets them aside)
  ArchiveFile plus[2];
  ArchiveFile files[2][3], lens[2], order[2];  // (a mate pass reads the order stream from its start: one handle each)
  scalce_read_fn rd[2][3];
  void *user[2][3];
  Archive(const Options &o, const std::string &path, int nm) {
    base[0] = base[1] = path;
    if (o.pairs() && !second_file(path, base[1])) FAIL("Cannot get file name for paired end for file %s.\n", path.c_str());
    // a variable-length archive has a length stream next to the other three: without the file, the reads come back padded
    for (int m = 0; m < nm; m++) {
      const std::string lpath = scalce_name(base[m], 'l');
      struct stat lst;
      if (stat(lpath.c_str(), &lst) != 0) continue;
      if (o.interleave) FAIL("%s: an archive of variable-length reads is decompressed mate by mate (-r), not interleaved (-i)\n", lpath.c_str());
      if (o.fasta || o.no_qual) FAIL("%s: an archive of variable-length reads is decompressed with its qualities, not with -Q / -f\n", lpath.c_str());
      has_lens[m] = true;
    }
    static const char ext[3] = {'r', 'n', 'q'};
    for (int m = 0; m < 2; m++)
      for (int k = 0; k < 3; k++) {
        rd[m][k] = m < nm ? ArchiveFile::read : nullptr;
        user[m][k] = &files[m][k];
        if (m < nm) files[m][k].open(scalce_name(base[m], ext[k]));
      }
    for (int m = 0; m < nm; m++)
      if (has_lens[m]) lens[m].open(scalce_name(base[m], 'l'));
    struct stat ost;
    has_order = !o.archive_order && stat(scalce_name(base[0], 'o').c_str(), &ost) == 0;
    if (has_order && o.has_range)
      FAIL("--records counts in the archive's order and %s holds the input's: give --archive-order with --records\n", scalce_name(base[0], 'o').c_str());
    for (int m = 0; m < (o.interleave ? 1 : nm) && has_order; m++) order[m].open(scalce_name(base[0], 'o'));
    // what follows the names: put back when every mate has its stream, names are printed and nothing sets the streams aside
    has_comments = !o.no_comments && o.use_names;
    for (int m = 0; m < nm && has_comments; m++) has_comments = side_file_present(scalce_name(base[m], 'c'));
    for (int m = 0; m < nm && has_comments; m++) comments[m].open(scalce_name(base[m], 'c'));
    // what the archive does not keep of the bases: put back when every mate has its stream
    has_exceptions = !o.stored_bases;
    for (int m = 0; m < nm && has_exceptions; m++) has_exceptions = side_file_present(scalce_name(base[m], 'x'));
    for (int m = 0; m < nm && has_exceptions; m++) exceptions[m].open(scalce_name(base[m], 'x'));
    // the '+' lines: put back when every mate has its stream and the records that go out have such a line
    has_plus = !o.bare_plus && !o.no_qual && !o.fasta;
    for (int m = 0; m < nm && has_plus; m++) has_plus = side_file_present(scalce_name(base[m], 'p'));
    for (int m = 0; m < nm && has_plus; m++) plus[m].open(scalce_name(base[m], 'p'));
  }
};
// One path for every archive: scalce_stream_decompress moves it through the device in windows of whole records.  The read
// callbacks hand out the files as they are read, the write callback writes each window's text as it arrives.
static int do_decompress(const Options &o, const std::string &path, scalce_ctx *ctx) {
  const double t0 = now();
  const int nm = o.pairs() ? 2 : 1;
  Archive ar(o, path, nm);
  const scalce_unpack_params p = unpack_params_from(o, nm, ar.lens, ar.has_lens);
  const scalce_unpack_range rg = unpack_range_from(o, nm, ar.files);
  // the digest stream, when the archive has one: what the input was, and whether the text asked for is the input's
  scalce_host::Digest dg;
  const std::string dpath = scalce_name(ar.base[0], 'd');
  struct stat dst;
  const bool has_digest = stat(dpath.c_str(), &dst) == 0;
  const char *unchecked = nullptr;
  if (has_digest) {
    ArchiveFile fd;
    fd.open(dpath);
    uint8_t raw[scalce_host::DIGEST_MAX_BYTES + 8];
    size_t have = 0;
    for (int64_t k; have < sizeof raw && (k = ArchiveFile::read(&fd, raw + have, sizeof raw - have)) != 0; have += (size_t)k)
      if (k < 0) FAIL("Read error on %s\n", dpath.c_str());
    if (const char *why = scalce_host::digest_read(raw, have, &dg)) {
      if (!strncmp(why, "is not", 6)) FAIL("%s %s\n", dpath.c_str(), why);
      FAIL("%s\n", why);
    }
    const int kind = dg.kind & 3, archive_texts = scalce_host::digest_kind_texts(dg.kind);
    if (dg.texts != archive_texts) {
      char msg[128];
      scalce_host::digest_count_message(msg, sizeof msg, (uint64_t)dg.texts, (uint64_t)archive_texts);
      FAIL("%s\n", msg);
    }
    const bool two_line = (dg.kind & scalce_host::DIGEST_KIND_FASTA) != 0;
    unchecked = o.has_range ? "--records" : o.archive_order ? "--archive-order" : o.no_comments ? "--no-comments" : o.stored_bases ? "--stored-bases" :
                o.bare_plus ? "--bare-plus" : !o.use_names ? "-n" : o.no_qual ? "-Q" :
                kind == scalce_host::DIGEST_KIND_PAIRED && !o.paired ? (o.interleave ? "-i: the input was two files" : "the input was two files: give -r") :
                kind == scalce_host::DIGEST_KIND_INTERLEAVED && !o.interleave ? (o.paired ? "-r: the input was one interleaved file" : "the input was interleaved: give -i") :
                kind == scalce_host::DIGEST_KIND_SINGLE && o.pairs() ? "the input was one single-end text" :
                two_line != o.fasta ? (two_line ? "the input was FASTA: give -f" : "-f: the input was FASTQ") :
                !ar.has_order ? "no .scalceo" : !ar.has_comments ? "no .scalcec" : !ar.has_exceptions ? "no .scalcex" : !two_line && !ar.has_plus ? "no .scalcep" : nullptr;
    if (unchecked && o.test) FAIL("--test: the text cannot be checked against the digest (%s)\n", unchecked);
  }
  scalce_unpack_params pd = p;
  pd.digest = has_digest && !unchecked;
  TextSink sink;
  sink.out = o.out; sink.split = o.split; sink.interleave = o.interleave; sink.discard = o.test;
  scalce_unpack_stats st;
  scalce_unpack_range_stats rs;
  scalce_restore_stats os;
  char err[1024] = "";
  std::string spill_dir;
  int rc;
  scalce_unpack_comments cm;
  memset(&cm, 0, sizeof cm);
  for (int m = 0; m < nm && ar.has_comments; m++) { cm.com_rd[m] = ArchiveFile::read; cm.com_user[m] = &ar.comments[m]; }
  scalce_unpack_exceptions ex;
  memset(&ex, 0, sizeof ex);
  for (int m = 0; m < nm && ar.has_exceptions; m++) { ex.exc_rd[m] = ArchiveFile::read; ex.exc_user[m] = &ar.exceptions[m]; }
  const scalce_unpack_comments *cmp = ar.has_comments ? &cm : nullptr;
  const scalce_unpack_exceptions *exp = ar.has_exceptions ? &ex : nullptr;
  scalce_unpack_plus pl;
  memset(&pl, 0, sizeof pl);
  for (int m = 0; m < nm && ar.has_plus; m++) { pl.plus_rd[m] = ArchiveFile::read; pl.plus_user[m] = &ar.plus[m]; }
  const scalce_unpack_plus *plp = ar.has_plus ? &pl : nullptr;
  const bool side = ar.has_comments || ar.has_exceptions || ar.has_plus;
  if (ar.has_order) {  // the input order back: two passes through a spill under -t, next to the output, or in $TMPDIR
    scalce_restore_params rp;
    memset(&rp, 0, sizeof rp);
    for (int m = 0; m < (o.interleave ? 1 : nm); m++) { rp.order_rd[m] = ArchiveFile::read; rp.order_user[m] = &ar.order[m]; }
    if (o.temp_given) {
      spill_dir = o.temp;
      struct stat tst;
      if (stat(spill_dir.c_str(), &tst) != 0 && mkdir(spill_dir.c_str(), 0777) != 0) FAIL("Cannot create temporary directory %s (-t)\n", spill_dir.c_str());
    } else if (o.out == "-" || o.out.empty()) {
      spill_dir = getenv("TMPDIR") && getenv("TMPDIR")[0] ? getenv("TMPDIR") : "/tmp";
    } else {
      const size_t sl = o.out.rfind('/');
      spill_dir = sl == std::string::npos ? "." : sl == 0 ? "/" : o.out.substr(0, sl);
    }
    rp.spill_dir = spill_dir.c_str();
    memset(&rs, 0, sizeof rs);
    // (side streams: the one entry point that takes comments, exceptions and '+' lines, any of them; else the call as it always was)
    rc = side ? scalce_stream_decompress_plus(ctx, &pd, cmp, exp, plp, nullptr, &rp, ar.rd, ar.user, TextSink::write, &sink, &st, nullptr, &os, err, sizeof err)
              : scalce_stream_decompress_restore(ctx, &pd, &rp, ar.rd, ar.user, TextSink::write, &sink, &st, &os, err, sizeof err);
  } else
    rc = side ? scalce_stream_decompress_plus(ctx, &pd, cmp, exp, plp, &rg, nullptr, ar.rd, ar.user, TextSink::write, &sink, &st, &rs, nullptr, err, sizeof err)
              : scalce_stream_decompress_range(ctx, &pd, &rg, ar.rd, ar.user, TextSink::write, &sink, &st, &rs, err, sizeof err);
  if (rc) {
    // (parts already written stay where they are)
    if (st.error_stream == 5 && st.error_mate >= 0 && !strncmp(err, "(ERROR) is not", 14))  // (a predicate about the comment stream's file)
      FAIL("%s %s\n", ar.comments[st.error_mate].path.c_str(), err + 8);
    if (st.error_stream == 6 && st.error_mate >= 0 && !strncmp(err, "(ERROR) is not", 14))  // (... about the exception stream's)
      FAIL("%s %s\n", ar.exceptions[st.error_mate].path.c_str(), err + 8);
    if (st.error_stream == 7 && st.error_mate >= 0 && !strncmp(err, "(ERROR) is not", 14))  // (... about the plus-line stream's)
      FAIL("%s %s\n", ar.plus[st.error_mate].path.c_str(), err + 8);
    if (st.error_wants_file && st.error_mate >= 0 && st.error_stream >= 0 && st.error_stream < 3)
      FAIL("%s %s\n", st.error_stream == 0 ? ar.base[st.error_mate].c_str() : ar.files[st.error_mate][st.error_stream].path.c_str(), err);
    fprintf(stderr, "%s%s\n", strncmp(err, "(ERROR)", 7) ? "(ERROR) " : "", err);
    exit(1);
  }
  for (int m = 0; m < (o.interleave ? 1 : nm); m++) sink.finish(m);
  LOG("\tTime elapsed: %.2f s (archive files read %.2f; qualities up and decoded %.2f; records to text %.2f; text down and written %.2f%s)\n",
      now() - t0, st.read_wait_s, st.decode_s, st.records_s, st.write_s, nm == 2 && !o.interleave ? ", one mate after the other" : "");
  LOG("\tWindows: %llu of up to %llu bytes of text; device memory held at most %llu bytes\n", (unsigned long long)st.windows,
      (unsigned long long)st.window_text_bytes, (unsigned long long)st.peak_device_bytes);
  if (ar.has_order) {
    LOG("\tOrder: %llu records restored through %llu stripes of up to %llu records; %llu bytes spilled in %s\n", (unsigned long long)os.records,
        (unsigned long long)os.stripes, (unsigned long long)os.stripe_records, (unsigned long long)os.spilled_bytes, spill_dir.c_str());
    LOG("\tOrder: window loop %.2f s (spill written %.2f), stripe loop %.2f s (spill read %.2f, waiting for place + permute %.2f)\n", os.group_pass_s,
        os.spill_write_s, os.stripe_pass_s, os.spill_read_s, os.place_wait_s);
  }
  if (o.has_range) {
    char total[32] = "unknown";
    if (rs.total_records != ~0ull) snprintf(total, sizeof total, "%llu", (unsigned long long)rs.total_records);
    LOG("\tRange: records %llu to %llu of %s; quality frames decoded %llu, passed over %llu\n", (unsigned long long)rs.first_record,
        (unsigned long long)(rs.first_record + rs.nrecords), total, (unsigned long long)(rs.frames_decoded[0] + rs.frames_decoded[1]),
        (unsigned long long)(rs.frames_passed[0] + rs.frames_passed[1]));
  }
  // the digest: what was written (or, under --test, only decoded) against what the input was, text by text
  if (!has_digest) {
    if (o.test) LOG("\tDigest: none recorded; streams decode to their end\n");
    return 0;
  }
  if (unchecked) { LOG("\tDigest: not checked (%s)\n", unchecked); return 0; }
  int bad = 0;
  for (int m = 0; m < dg.texts; m++) {
    scalce_host::DigestText got;
    got.bytes = st.text_bytes[m];
    got.crc = st.crc[m];
    if (got.bytes == dg.text[m].bytes && got.crc == dg.text[m].crc) {
      LOG("\tDigest: %llu bytes, crc32 %08x: the input's\n", (unsigned long long)got.bytes, got.crc);
      continue;
    }
    char msg[256];
    scalce_host::digest_mismatch_message(msg, sizeof msg, m + 1, dg.text[m], got);
    fprintf(stderr, "(ERROR) %s\n", msg);
    bad = 1;
  }
  return bad;
}

// ---- the command line ------------------------------------------------------------------------------------------
// The three numbers with a form of their own.  Each accepts what it always did, so they stay three.
static uint64_t bucket_set_size_arg(const char *arg) {  // -B NUM[M|G]
  std::string s = arg;
  const char al = s.empty() ? 0 : s.back();
  uint64_t unit = 1024 * 1024ull;
  if (al == 'G') unit *= 1024; else if (al != 'M') FAIL("Size parameter must be ended with G or M.\n");
  s.pop_back();
  return unit * (uint64_t)atoi(s.c_str());
}
static uint64_t window_arg(const char *arg) {  // --window NUM[K|M|G]
  char *e = nullptr;
  const unsigned long long v = strtoull(arg, &e, 10);
  const uint64_t unit = *e == 'K' ? 1ull << 10 : *e == 'M' ? 1ull << 20 : *e == 'G' ? 1ull << 30 : 1;
  if (e == arg || !v || (*e && (unit == 1 || e[1]))) FAIL("--window takes a positive number of bytes, optionally ended with K, M or G.\n");
  return v * unit;
}
static void records_arg(const char *arg, Options &o) {  // --records FIRST[:COUNT]
  // both plain decimal numbers (strtoull alone would take a sign, blanks and an empty string)
  auto number = [](const char *b, const char *e, uint64_t &v) {
    if (b == e || e - b > 19) return false;
    v = 0;
    for (; b != e; b++) { if (*b < '0' || *b > '9') return false; v = v * 10 + (uint64_t)(*b - '0'); }
    return true;
  };
  const char *colon = strchr(arg, ':'), *end = arg + strlen(arg);
  if (!number(arg, colon ? colon : end, o.range_first) || (colon && !number(colon + 1, end, o.range_count)))
    FAIL("--records takes FIRST or FIRST:COUNT, two non-negative numbers of records.\n");
  o.has_range = true;
}
// false: the run ends here with status 0 (-v, -h, an unknown option)
static bool parse_options(int argc, char **argv, Options &o) {
  static struct option long_opt[] = {{"help", 0, 0, 'h'}, {"lossy-percentage", 1, 0, 'p'}, {"decompress", 0, 0, 'd'},
                                     {"compression", 1, 0, 'c'}, {"output", 1, 0, 'o'}, {"sample-size", 1, 0, 's'},
                                     {"no-qualities", 0, 0, 'Q'}, {"patterns", 1, 0, 'P'}, {"temp-directory", 1, 0, 't'},
                                     {"bucket-set-size", 1, 0, 'B'}, {"paired-end", 0, 0, 'r'}, {"skip-names", 1, 0, 'n'},
                                     {"split-reads", 1, 0, 'S'}, {"fasta", 0, 0, 'f'}, {"threads", 1, 0, 'T'},
                                     {"version", 0, 0, 'v'}, {"no-arithmetic", 0, 0, 'A'}, {"patterns-bin", 1, 0, 1000},
                                     {"gpus", 1, 0, 1001}, {"interleave", 0, 0, 'i'}, {"window", 1, 0, 1002},
                                     {"records", 1, 0, 1003}, {"variable-length", 0, 0, 1004},
                                     {"max-length", 1, 0, 1005}, {"keep-order", 0, 0, 1006},
                                     {"archive-order", 0, 0, 1007}, {"keep-comments", 0, 0, 1008},
                                     {"no-comments", 0, 0, 1009}, {"keep-bases", 0, 0, 1010},
                                     {"stored-bases", 0, 0, 1011}, {"keep-plus", 0, 0, 1012},
                                     {"bare-plus", 0, 0, 1013}, {"lossless", 0, 0, 1014},
                                     {"digest", 0, 0, 1015}, {"test", 0, 0, 1016}, {0, 0, 0, 0}};
  int opt;
  while ((opt = getopt_long(argc, argv, "vhp:T:dc:o:fs:t:B:rQAn:P:S:i", long_opt, 0)) != -1) {
    switch (opt) {
      case 'v': return false;
      case 'h': fputs(HELP_TEXT, stdout); return false;
      case 'A': o.no_ac = true; break;
      case 'f': o.fasta = true; break;
      case 'Q': o.no_qual = true; break;
      case 'c':
        if (!strcmp(optarg, "gz") || !strcmp(optarg, "pigz")) o.container = 1;
        else if (!strcmp(optarg, "no")) o.container = 0;
        else if (!strcmp(optarg, "bz")) FAIL("bzip2 containers are outside this build's scope (SURVEY.md section 2, #18: host-side container code); use gz or no\n");
        else FAIL("Unknown compression mode. See help for details.\n");
        break;
      case 'B': o.bucket_set_size = bucket_set_size_arg(optarg); break;
      case 'p': o.lossy = atoi(optarg); break;
      case 'T': o.threads = atoi(optarg); break;
      case 'S': o.split = atoi(optarg); break;
      case 'r': o.paired = true; break;
      case 'i': o.interleave = true; break;
      case 's': o.sample = atoi(optarg); break;
      case 'd': o.decompress = true; break;
      case 'P': o.patterns = optarg; break;
      case 't': o.temp = optarg; o.temp_given = true; break;
      case 'o': o.out = optarg; break;
      case 'n': o.use_names = false; o.library = optarg; break;
      case 1000: o.patterns_bin = optarg; break;
      case 1001: o.gpus = atoi(optarg); break;
      case 1002: o.window = window_arg(optarg); break;
      case 1003: records_arg(optarg, o); break;
      case 1004: o.varlen = true; break;
      case 1005:
        o.max_length = atoi(optarg);
        if (o.max_length < 1 || o.max_length > 2498) FAIL("--max-length takes the longest read's number of bases, 1 to 2498.\n");
        o.varlen = true;
        break;
      case 1006: o.keep_order = true; break;
      case 1007: o.archive_order = true; break;
      case 1008: o.keep_comments = true; break;
      case 1009: o.no_comments = true; break;
      case 1010: o.keep_bases = true; break;
      case 1011: o.stored_bases = true; break;
      case 1012: o.keep_plus = true; break;
      case 1013: o.bare_plus = true; break;
      case 1014: o.lossless = true; break;
      case 1015: o.digest = true; break;
      case 1016: o.test = true; break;
      default: fputs(HELP_TEXT, stdout); return false;
    }
  }
  if (o.lossless) {  // (FASTA has no '+' line: there the three are the input)
    o.keep_order = o.keep_comments = o.keep_bases = true;
    if (!o.fasta) o.keep_plus = true;
  }
  return true;
}
// check_arguments, main.cpp:120-164, and what this build refuses; all of it before anything touches a device
static void check_arguments(const Options &o, const std::vector<std::string> &files) {
  if (o.interleave && o.paired) FAIL("Interleaved option (-i) cannot be used with paired-end option (-r).\n");
  if (o.digest && o.decompress) FAIL("--digest is an option of compression: -d checks the text by itself when the archive has a .scalced\n");
  if (o.digest && !o.lossless) FAIL("--digest needs --lossless: only then is the text -d writes the input's\n");
  if (o.test) {  // (-o is not needed and is ignored)
    if (!o.decompress) FAIL("--test can be only used with decompression (-d).\n");
    const char *other = o.archive_order ? "--archive-order" : o.no_comments ? "--no-comments" : o.stored_bases ? "--stored-bases" : o.bare_plus ? "--bare-plus" :
                        !o.use_names ? "-n" : o.no_qual ? "-Q" : o.has_range ? "--records" : nullptr;
    if (other) FAIL("--test checks that the archive gives the input's text back: %s asks for another text\n", other);
  }
  if (o.out.empty() && !o.test) FAIL("No output file specified.\n");
  if (!o.use_names && o.library.empty()) FAIL("No library name specified.\n");
  if (o.has_range && !o.decompress) FAIL("--records can be only used with decompression (-d).\n");
  if (o.lossless) {  // (in front of the single options' refusals: each of these says why the promise cannot be kept)
    if (o.decompress) FAIL("--lossless is an option of compression: -d puts everything back by itself when the archive has the streams\n");
    if (o.lossy != 0) FAIL("--lossless with -p %d: the lossy quality transform changes qualities, the input would not come back\n", o.lossy);
    if (!o.use_names) FAIL("--lossless with -n: names that are not kept cannot come back\n");
    if (o.no_qual) FAIL("--lossless with -Q: qualities that are not kept cannot come back\n");
    if (o.gpus > 1) FAIL("--lossless runs on one GPU: with --gpus %d the order, comments, exceptions and '+' lines lie spread over the ranks\n", o.gpus);
  }
  if (o.keep_plus && o.decompress) FAIL("--keep-plus is an option of compression: -d puts the '+' lines back by itself when the archive has a .scalcep\n");
  if (o.bare_plus && !o.decompress) FAIL("--bare-plus can be only used with decompression (-d).\n");
  if (o.keep_plus && o.fasta) FAIL("--keep-plus with -f: FASTA records have no '+' line to keep\n");
  if (o.keep_plus && o.no_qual) FAIL("--keep-plus with -Q: the records are kept as two lines, there is no '+' line to keep\n");
  if (o.keep_plus && o.gpus > 1) FAIL("--keep-plus runs on one GPU: with --gpus %d the '+' lines lie spread over the ranks\n", o.gpus);
  if (o.keep_order && o.decompress) FAIL("--keep-order is an option of compression: -d restores the order by itself when the archive has a .scalceo\n");
  if (o.archive_order && !o.decompress) FAIL("--archive-order can be only used with decompression (-d).\n");
  if (o.keep_order && o.gpus > 1) FAIL("--keep-order runs on one GPU: with --gpus %d the permutation lies spread over the ranks\n", o.gpus);
  if (o.keep_comments && o.decompress) FAIL("--keep-comments is an option of compression: -d puts the comments back by itself when the archive has a .scalcec\n");
  if (o.no_comments && !o.decompress) FAIL("--no-comments can be only used with decompression (-d).\n");
  if (o.keep_comments && !o.use_names) FAIL("--keep-comments with -n: nothing is kept for what follows a name that is not kept\n");
  if (o.keep_comments && o.gpus > 1) FAIL("--keep-comments runs on one GPU: with --gpus %d the comments lie spread over the ranks\n", o.gpus);
  if (o.keep_bases && o.decompress) FAIL("--keep-bases is an option of compression: -d puts the bases back by itself when the archive has a .scalcex\n");
  if (o.stored_bases && !o.decompress) FAIL("--stored-bases can be only used with decompression (-d).\n");
  if (o.keep_bases && o.gpus > 1) FAIL("--keep-bases runs on one GPU: with --gpus %d the exceptions lie spread over the ranks\n", o.gpus);
  if (o.decompress && files.size() > 1) FAIL("Too many files specified (decompression only supports one file).\n");
  if (o.lossy < 0 || o.lossy > 100) FAIL("Percentage must be in range [0,100].\n");
  if (o.out == "-" && !o.test && (o.split || o.paired)) FAIL("stdout can be only used with single-end file decompression. It cannot be used with --split-reads option!\n");
  if (files.empty()) FAIL("No input file specified.\n");
  for (auto &f : files)
    for (int m = 0; m < (o.paired ? 2 : 1); m++) {
      const std::string path = mate_file(f, m);
      struct stat st;
      if (stat(path.c_str(), &st) != 0) FAIL("File %s does not exist or it is not accessible.\n", path.c_str());
    }
  if (o.gpus > 1 && !o.decompress && (o.fasta || o.no_qual))
    FAIL("-f / -Q runs on one GPU: --gpus %d is not available without qualities\n", o.gpus);
  if (o.varlen && !o.decompress) {  // refused before anything touches a device
    if (o.interleave) FAIL("--variable-length is not available for interleaved input (-i): give the mates as two files (-r)\n");
    if (o.fasta) FAIL("--variable-length is not available for FASTA input (-f)\n");
    if (o.no_qual) FAIL("--variable-length is not available without qualities (-Q)\n");
    if (o.gpus > 1) FAIL("--variable-length runs on one GPU: --gpus %d is not available for reads of different lengths\n", o.gpus);
  }
  if (o.gpus > 1 && !o.decompress && o.interleave)
    FAIL("-i runs on one GPU: --gpus %d is not available for interleaved input\n", o.gpus);
}

int main(int argc, char **argv) {
  const double t_main = now();
  Options o;
  LOG("SCALCE %s [MI355X / HIP]\n", SCALCE_VERSION);
  if (!parse_options(argc, argv, o)) return 0;
  const std::vector<std::string> files(argv + optind, argv + argc);
  check_arguments(o, files);
  if (o.gpus > 1 && !o.decompress) {  // forks before anything touches a GPU
    // (a run that -B does not cut anywhere is one chunk: scalce_sharded_compress sends all its rows to rank 0)
    return multi_gpu_compress(o, files, argv[0]);
  }
  std::vector<uint8_t> table;
  bool is_text = false;
  scalce_ctx *ctx = open_device(o, argv[0], 0, table, is_text);
  set_threads(o.threads, 1);
  const double t_ready = now();
  const int rc = o.decompress ? do_decompress(o, files[0], ctx) : do_compress(o, files, ctx);
  scalce_ctx_destroy(ctx);
  LOG("\tProcess: device and core table ready %.2f s after main() began, %.2f s in all\n", t_ready - t_main, now() - t_main);
  LOG("Done!\n");
  return rc;
}
