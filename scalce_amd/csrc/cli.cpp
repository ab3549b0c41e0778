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
#include <getopt.h>
#include <hip/hip_runtime_api.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <sys/time.h>
#include <zlib.h>
#include <atomic>
#include <memory>
#include <thread>
#include <algorithm>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cerrno>
#include <csignal>

#include "../../include/scalce_hip.h"
#include "hip_own.hpp"
#include "pargz.hpp"
#include "lenstream.hpp"


#ifndef SCALCE_VERSION
#define SCALCE_VERSION "2.8-mi355x"
#endif

static void LOG(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
}
[[noreturn]] static void FAIL(const char *fmt, ...) {  // ERROR(), const.h:77-81
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "(ERROR) ");
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  exit(1);
}
static double now() {
  struct timeval t;
  gettimeofday(&t, 0);
  return t.tv_sec + 1e-6 * t.tv_usec;
}

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
    "  -p, --lossy-percentage INT  lossy quality transform, 0..100 (default 0)\n"
    "  -s, --sample-size INT       records sampled for the quality model (default 100000)\n"
    "  -B, --bucket-set-size NUM[M|G]  bucket storage that triggers a spill chunk (default 4G); order follows the reference\n"
    "  -P, --patterns FILE         text list of cores instead of the built-in table\n"
    "  -T, --threads INT           host threads that read plain input and deflate the gz containers (default: cores - 1,\n"
    "                              at most 64);\n"
    "                              the hot path itself runs on the GPU\n"
    "  -t, --temp-directory STR    accepted for compatibility (nothing is spilled)\n"
    "  -S, --split-reads INT       decompression: reads per output part\n"
    "      --window NUM[K|M|G]     decompression: bytes of FASTQ text per window (default 1G; -Q counts a record as its FASTQ).  The archive moves through the\n"
    "                              device in windows of whole records -- at least one record each --, so memory follows the\n"
    "                              window, not the archive, and -o - writes each window as it arrives\n"
    "      --records FIRST[:COUNT] decompression: only COUNT records (pairs under -r / -i; to the end without COUNT) from record\n"
    "                              FIRST on, counted from 0 in the order -d writes them.  What lies in front is passed over, not\n"
    "                              decoded (plain files seek); -S parts and made-up names (-n) count from FIRST; a file that\n"
    "                              is cut short behind the range is not noticed\n"
    "  -d, --decompress    -v, --version    -h, --help\n"
    "      --gpus N                compress on N GPUs, one process each, into ONE archive that is byte for byte the archive of\n"
    "                              one GPU (and of the reference at -T 1 with the same -B); input: one plain FASTQ file (pair), -c no\n"
    "core table: --patterns-bin FILE or $SCALCE_PATTERNS or patterns.bin next to the executable\n";

// ---- small I/O helpers ------------------------------------------------------------------------------
// Host threads: -T, else the cores shared by `procs` processes (a process alone leaves one to its main thread), at most
// 64.  Plain files are read by up to 8 of them, gzip members inflated by up to 32, the gz containers deflated by all.
static int g_threads = 1;
static void set_threads(const Options &o, int procs) {
  const int hw = (int)std::thread::hardware_concurrency();
  g_threads = o.threads > 0 ? o.threads : std::max(1, std::min(64, procs > 1 ? hw / procs : hw - 1));
}
static int g_threads_io() { return std::max(1, std::min(g_threads, 8)); }
static int g_threads_gz() { return std::max(1, std::min(g_threads, 32)); }

static bool is_gzip(const std::string &path) {  // the gzip magic (the reference's readers sniff it too, decompress.cpp:99-113)
  const int fd = ::open(path.c_str(), O_RDONLY);
  uint8_t mg[2] = {0, 0};
  const bool gz = fd >= 0 && ::pread(fd, mg, 2, 0) == 2 && mg[0] == 0x1F && mg[1] == 0x8B;
  if (fd >= 0) ::close(fd);
  return gz;
}
// fn(a, b) on the slices [a, b) of [0, n), `slice` bytes each, taken in turn by up to `threads` threads (the caller's included)
template <class Fn> static void for_slices(uint64_t n, uint64_t slice, int threads, Fn fn) {
  std::atomic<uint64_t> next{0};
  auto work = [&]() { for (uint64_t a; (a = next.fetch_add(slice)) < n;) fn(a, std::min(n, a + slice)); };
  const int nt = (int)std::min<uint64_t>((uint64_t)std::max(1, threads), (n + slice - 1) / slice);
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; t++) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
}
// n bytes of fd from offset off, read in slices by several threads (one thread copying out of the page cache delivers about
// 5 GB/s, a tenth of what an upload behind it can take)
static bool pread_parallel(int fd, uint8_t *dst, uint64_t n, uint64_t off, uint64_t slice, int threads) {
  std::atomic<bool> bad{false};
  for_slices(n, slice, threads, [&](uint64_t a, uint64_t b) {
    for (uint64_t done = a; done < b && !bad;) {
      const ssize_t k = ::pread(fd, dst + done, (size_t)(b - done), (off_t)(off + done));
      if (k <= 0) bad = true; else done += (uint64_t)k;
    }
  });
  return !bad;
}
// A whole file: plain by parallel pread, gzip (the IO_GZIP reader, compress.cpp:756) with its members inflated by several
// threads (our own -c gz containers are 4 MiB members)
static std::vector<uint8_t> read_whole(const std::string &path) {
  std::vector<uint8_t> out;
  if (is_gzip(path)) {
    scalce_host::ParGz z;
    if (!z.open(path, g_threads_gz())) FAIL("Cannot read file %s\n", path.c_str());
    std::vector<uint8_t> chunk(64u << 20);
    for (int64_t k; (k = z.read(chunk.data(), chunk.size())) != 0;) {
      if (k < 0) FAIL("Read error on %s\n", path.c_str());
      out.insert(out.end(), chunk.begin(), chunk.begin() + k);
    }
    return out;
  }
  const int fd = ::open(path.c_str(), O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) FAIL("Cannot read file %s\n", path.c_str());
  out.resize((size_t)st.st_size);
  if (!pread_parallel(fd, out.data(), out.size(), 0, 64u << 20, g_threads_io())) FAIL("Read error on %s\n", path.c_str());
  ::close(fd);
  return out;
}
static bool second_file(const std::string &p, std::string &out) {  // get_second_file, const.cpp:51-64
  out = p;
  for (int i = (int)out.size() - 1; i >= 0; i--)
    if (out[i] == '1') { out[i] = '2'; return true; }
  return false;
}
static std::string mate_file(const std::string &f, int m) {  // input f's file of mate m
  std::string out = f;
  if (m && !second_file(f, out)) FAIL("Cannot get file name for paired end for file %s. File should contain character 1.\n", f.c_str());
  return out;
}

// ---- the archive: the file headers of combine_and_compress_with_split (compress.cpp:263-343) ---------------------------
//   PREFIX_<m>.scalcer  magic, int32 no_ac (-A), int32 read length; the read stream (mate 1: buckets, each opened by
//                       [int32 core][int64 records]; mate 2: bare records in mate 1's order)
//   PREFIX_<m>.scalcen  magic, u8 names; the name stream, or without names (-n) int64 0 and the library name
//   PREFIX_<m>.scalcel  --variable-length only (lenstream.hpp): magic, int32 entry width, int32 L, one entry L - length per record
//   PREFIX_<m>.scalceq  magic, int64 Phred offset (mate 1's for both mates, compress.cpp:294,816-817); arithmetic coded:
//                       the scaled table (QTABLE_WORDS x u32), the int64 symbol count and the coded blocks; -A: the q' rows
static const uint8_t MAGIC[8] = {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'};
static constexpr size_t QTABLE_WORDS = 512000;
static std::string archive_path(const std::string &out, int m, char ext) { return out + "_" + std::to_string(m + 1) + ".scalce" + ext; }
// -c gz holds every file in a gzip container but an arithmetic-coded .scalceq (compress.cpp:249)
static bool gz_container(const Options &o, char ext) { return o.container == 1 && (ext != 'q' || o.no_ac); }
static std::vector<uint8_t> with_magic(const void *fields, size_t n) {
  std::vector<uint8_t> h(MAGIC, MAGIC + 8);
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

// Output file.  Plain: stdio.  gzip container (-c gz / pigz): the reference hands the stream to a pigz child or to
// zlib's gzwrite (buffio.cpp:148-188, 190-260); here the bytes are collected and deflated at close() by g_threads
// host threads, 4 MiB per independent gzip member -- concatenated members are one valid gzip file, which the
// reference's reader (gzread, decompress.cpp:99-113) and ours accept alike (once the hot path is on
// the GPU, single-threaded deflate of .scalcer/.scalcen is what the wall clock of a run is made of).
struct OutFile {
  bool gz = false;
  FILE *f = nullptr;
  std::vector<uint8_t> pending;  // gz only: bytes not deflated yet
  uint64_t written = 0;
  static constexpr size_t MEMBER = 4u << 20;
  void open(const std::string &path, bool gz_) {
    gz = gz_;
    f = path == "-" ? stdout : fopen(path.c_str(), "wb");
    if (!f) FAIL("Cannot create %s\n", path.c_str());
  }
  void raw(const uint8_t *b, size_t n) {
    written += n;
    while (n) {
      size_t k = n > (1u << 30) ? (1u << 30) : n;
      if (fwrite(b, 1, k, f) != k) FAIL("write failed\n");
      b += k; n -= k;
    }
  }
  void write(const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    if (!gz) { raw(b, n); return; }
    pending.insert(pending.end(), b, b + n);
    // enough for every thread: deflate what is there, member by member (the stream never has to sit in memory whole)
    if (pending.size() >= MEMBER * (size_t)std::max(1, g_threads) * 2) flush_members(false);
  }
  void write(const std::vector<uint8_t> &v) { write(v.data(), v.size()); }
  // The reference writes its containers at zlib's default level (buffio.cpp: gzopen(path, "wb")), and so does this writer for
  // what deflate shrinks (names: to a third).  The read stream is 2-bit packed bases, as good as incompressible (the
  // reference's own gz gains 2.5 % on it) and the slowest thing zlib can be fed: ~20 MB/s per core at level 6 -- 3.6 of the
  // 5.8 s of a 50 M-read run with -c gz.  A member none of whose sample windows (eight of 16 KiB, spread over the member)
  // shrinks by a tenth at level 1 is therefore Huffman-coded only (Z_HUFFMAN_ONLY: no match search, ~15 x the speed, within
  // a percent of the size).  SCALCE_GZ_LEVEL=<n> turns that off and deflates every member at level n.
  static bool hardly_compressible(const uint8_t *src, size_t n) {
    static const bool off = getenv("SCALCE_GZ_LEVEL") != nullptr;   // (a level asked for by hand is applied to every member)
    if (off || n < 4096) return false;
    const size_t win = std::min<size_t>(n, 16u << 10), nwin = n >= 8 * win ? 8 : 1;
    std::vector<uint8_t> tmp(compressBound((uLong)win));
    for (size_t i = 0; i < nwin; i++) {
      const size_t at = nwin == 1 ? 0 : (n - win) / (nwin - 1) * i;
      uLongf got = (uLongf)tmp.size();
      if (compress2(tmp.data(), &got, src + at, (uLong)win, 1) != Z_OK) return false;
      if (got * 10 < win * 9) return false;   // this part does shrink: the member goes through deflate proper
    }
    return true;
  }
  static void deflate_member(const uint8_t *src, size_t n, std::vector<uint8_t> &out) {
    z_stream z;
    memset(&z, 0, sizeof z);
    const bool fast = n && hardly_compressible(src, n);
    // (what does shrink -- names -- goes at zlib's default level, the reference's: level 3 is 2.4 x the speed for a tenth more
    //  bytes of that stream; SCALCE_GZ_LEVEL=3 asks for it)
    static const int level = getenv("SCALCE_GZ_LEVEL") ? atoi(getenv("SCALCE_GZ_LEVEL")) : Z_DEFAULT_COMPRESSION;
    if (deflateInit2(&z, fast ? 1 : level, Z_DEFLATED, 15 + 16, 8, fast ? Z_HUFFMAN_ONLY : Z_DEFAULT_STRATEGY) != Z_OK) FAIL("deflateInit2 failed\n");
    out.resize(deflateBound(&z, (uLong)n) + 64);
    z.next_in = const_cast<Bytef *>(src); z.avail_in = (uInt)n;
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) FAIL("deflate failed\n");
    out.resize(z.total_out);
    deflateEnd(&z);
  }
  void flush_members(bool all) {
    const size_t whole = pending.size() / MEMBER, nchunks = all ? (pending.empty() ? 0 : (pending.size() + MEMBER - 1) / MEMBER) : whole;
    if (!nchunks) return;
    std::vector<std::vector<uint8_t>> members(nchunks);
    const size_t done = std::min(pending.size(), nchunks * MEMBER);
    for_slices(done, MEMBER, g_threads, [&](uint64_t a, uint64_t b) { deflate_member(pending.data() + a, b - a, members[a / MEMBER]); });
    for (auto &m : members) raw(m.data(), m.size());
    pending.erase(pending.begin(), pending.begin() + done);
  }
  void close() {
    if (gz && f) {
      const bool nothing = written == 0 && pending.empty();
      flush_members(true);
      if (nothing) { std::vector<uint8_t> m; deflate_member(nullptr, 0, m); raw(m.data(), m.size()); }  // an empty gzip file
      pending.clear(); pending.shrink_to_fit();
    }
    if (f && f != stdout) fclose(f);
    f = nullptr;
  }
};
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

// One mate's input: the files of the command line one after the other (compress.cpp:756-797 runs them through the same
// trie; the record stream is their concatenation), each plain or gzip (the reference opens everything through zlib,
// :767-779).  Plain files are read by parallel pread straight into the pinned chunk the streaming host hands in.
struct MateSource {
  std::vector<std::string> files;
  size_t cur = 0;
  int fd = -1;
  scalce_host::ParGz pgz;     // gzip input: members inflated on several threads (pargz.hpp)
  bool gz = false;
  std::vector<uint8_t> peek;  // bytes read ahead for the quality sample, served first
  size_t peek_pos = 0;
  bool open_next() {
    if (cur >= files.size()) return false;
    const std::string &path = files[cur++];
    if (is_gzip(path)) {
      if (!pgz.open(path, std::max(1, g_threads))) FAIL("Cannot read file %s\n", path.c_str());
      gz = true;
      return true;
    }
    fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) FAIL("Cannot read file %s\n", path.c_str());
#ifdef POSIX_FADV_SEQUENTIAL
    posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
#endif
    return true;
  }
  uint64_t fpos = 0;  // plain files: where the next read starts
  bool hold_at_file_end = false;  // fill_peek: the sample never runs into the next file
  // The reference reads every file on its own, line by line (compress.cpp:756-811, gzgets): a file whose last line has no
  // newline still ends there.  Concatenated byte-wise that line would run into the next file's '@name', so a file that
  // does not end in a newline is given one.
  uint8_t last_byte = '\n';
  bool pending_newline = false;
  // -i: every file must hold whole pairs (concatenated, a file with an odd record count would pair the next file's records
  // the wrong way round).  pair_lines = lines of a pair; the newlines of the current file are counted on their way through.
  uint64_t pair_lines = 0, file_lines = 0;
  std::string error;  // why read_raw returned -1, when it was the input's shape
  int64_t read_raw(void *dst, uint64_t cap) {
    for (;;) {
      if (pending_newline && cap) { pending_newline = false; last_byte = '\n'; *static_cast<uint8_t *>(dst) = '\n'; return 1; }
      if (fd < 0 && !gz) {
        if (hold_at_file_end && cur >= 1) return 0;
        if (!open_next()) return 0;
        fpos = 0;
        file_lines = 0;
      }
      const int64_t k = gz ? pgz.read(dst, cap) : read_plain(static_cast<uint8_t *>(dst), cap);
      if (k < 0) return -1;
      if (k > 0) {
        const uint8_t *p = static_cast<const uint8_t *>(dst), *e = p + k;
        if (pair_lines)
          while ((p = static_cast<const uint8_t *>(memchr(p, '\n', (size_t)(e - p))))) { file_lines++; p++; }
        last_byte = static_cast<uint8_t *>(dst)[k - 1];
        return k;
      }
      if (gz) { pgz.close(); gz = false; } else { ::close(fd); fd = -1; }
      if (last_byte != '\n') pending_newline = true;
      const uint64_t lines = file_lines + (pending_newline ? 1 : 0), lpr = pair_lines / 2;
      if (pair_lines && lines % pair_lines && lines % lpr == 0) {
        char msg[4352];
        snprintf(msg, sizeof msg, "(ERROR) %s holds an odd number of records (%llu): -i needs mate 1 and mate 2 of every pair\n",
                 files[cur - 1].c_str(), (unsigned long long)(lines / lpr));
        error = msg;
        return -1;
      }
    }
  }
  // a big request on a plain file is read by several threads at once
  int64_t read_plain(uint8_t *dst, uint64_t cap) {
    struct stat st;
    if (fstat(fd, &st) != 0) return -1;
    const uint64_t want = std::min(cap, (uint64_t)st.st_size > fpos ? (uint64_t)st.st_size - fpos : 0);
    if (!pread_parallel(fd, dst, want, fpos, 16u << 20, g_threads_io())) return -1;
    fpos += want;
    return (int64_t)want;
  }
  int64_t read(void *dst, uint64_t cap) {
    if (peek_pos < peek.size()) {
      const size_t k = (size_t)std::min<uint64_t>(cap, peek.size() - peek_pos);
      memcpy(dst, peek.data() + peek_pos, k);
      peek_pos += k;
      if (peek_pos == peek.size()) { std::vector<uint8_t>().swap(peek); peek_pos = 0; }
      return (int64_t)k;
    }
    return read_raw(dst, cap);
  }
  // read ahead until the text holds `records` records or the FIRST file ends: quality_mapping_init's sample is taken
  // from files[0] alone (get_quality_stats, compress.cpp:761; the loop of qualities.cpp:66-78 stops at its end)
  void fill_peek(int records, int lines_per_record) {
    hold_at_file_end = true;
    const size_t want = (size_t)lines_per_record * (size_t)records;
    size_t lines = 0, scanned = 0;
    for (int64_t got = 1; got;) {
      const uint8_t *p = peek.data();
      while (scanned < peek.size() && lines < want) {
        const void *nl = memchr(p + scanned, '\n', peek.size() - scanned);
        if (!nl) { scanned = peek.size(); break; }
        scanned = (size_t)((const uint8_t *)nl - p) + 1;
        lines++;
      }
      if (lines >= want) break;
      const size_t old = peek.size(), step = 16u << 20;
      peek.resize(old + step);
      for (got = 0; (size_t)got < step;) {
        const int64_t k = read_raw(peek.data() + old + got, step - (size_t)got);
        if (k < 0) FAIL("%s", error.empty() ? "Read error\n" : error.c_str());
        if (k == 0) break;
        got += k;
      }
      peek.resize(old + (size_t)got);
    }
    hold_at_file_end = false;
  }
  static int64_t read_cb(void *user, void *dst, uint64_t cap) { return static_cast<MateSource *>(user)->read(dst, cap); }
};

// sampling loop of quality_mapping_init (qualities.cpp:64-97) on the text read ahead: the first `sample` records r with
// r % stride == first (-i: stride 2, `first` = the mate -- the _interleave == 10 / 20 skips of qualities.cpp:67-90)
static void sample_stats(const uint8_t *t, size_t n, int sample, int32_t stat[128], int &read_length, int stride = 1, int first = 0) {
  size_t line[5] = {0};  // where a record's four lines start, and the next record
  for (long r = 0, taken = 0; taken < sample; r++, line[0] = line[4]) {
    for (int k = 1; k < 5; k++) {
      const void *nl = line[k - 1] < n ? memchr(t + line[k - 1], '\n', n - line[k - 1]) : nullptr;
      if (!nl) return;
      line[k] = (size_t)((const uint8_t *)nl - t) + 1;
    }
    if (r % stride != first) continue;
    taken++;
    for (size_t j = line[3]; j + 1 < line[4]; j++) stat[t[j] & 127]++;
    read_length = (int)(line[4] - 1 - line[3]);
  }
}

// ---- run setup --------------------------------------------------------------------------------------------
static scalce_params params_from(const Options &o) {
  scalce_params p;
  scalce_params_default(&p);
  p.paired = o.pairs(); p.use_names = o.use_names; p.no_ac = o.no_ac; p.bucket_set_size = o.bucket_set_size;
  p.fasta = o.fasta; p.no_qualities = o.no_qual; p.interleaved = o.interleave;
  p.variable_length = o.varlen;
  return p;
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
static int do_compress(const Options &o, const std::vector<std::string> &files, scalce_ctx *ctx) {
  const double t0 = now();
  const int nm = o.pairs() ? 2 : 1;
  const int nsrc = o.interleave ? 1 : nm;  // input streams: -i reads both mates from one
  uint64_t original = 0, bytes1 = 0;  // input bytes: every mate's, mate 1's
  bool plain1 = true;                 // no gzip among mate 1's files
  scalce_params p = params_from(o);
  const bool no_qual = o.fasta || o.no_qual;
  LOG("Preprocessing FASTQ files ...\n");
  MateSource src[2];
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
  // rows to expect: exact enough for plain text (a record is 2 L + 6 bytes plus its name), unknown behind gzip
  const uint64_t hint = plain1 ? bytes1 / ((o.fasta ? 1 : 2) * (uint64_t)p.read_len[0] + (o.fasta ? 4 : 8)) / (o.interleave ? 2 : 1) + 64 : 0;
  uint64_t piece = 256ull << 20;  // per chunk; three of them are pinned per mate
  if (const char *e = getenv("SCALCE_PIECE_BYTES")) piece = strtoull(e, nullptr, 10);
  if (hint && bytes1 + (1u << 20) < piece) piece = bytes1 + (1u << 20);  // small inputs: no point in pinning gigabytes
  scalce_batch *b = nullptr;
  scalce_stream_stats ss;
  char emsg[512] = "";
  const double t1 = now();
  if (scalce_stream_compress(ctx, &p, MateSource::read_cb, &src[0], nsrc == 2 ? MateSource::read_cb : nullptr, nsrc == 2 ? &src[1] : nullptr, piece,
                             hint, SCALCE_STREAM_LEAN | SCALCE_STREAM_DEFER_ENTROPY, &b, &ss, emsg, sizeof emsg)) {
    if (!src[0].error.empty()) fputs(src[0].error.c_str(), stderr);  // (-i: a file of odd record count; the stream only saw a read error)
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
  per_mate([&](int m) {
    downs[m].reset(new Downloader);
    OutFile fR, fN;
    fR.open(archive_path(o.out, m, 'r'), gz_container(o, 'r'));
    fR.write(reads_header(o, p.read_len[m]));
    downs[m]->to_file(ctx, b, SCALCE_OUT_READS, m, fR);
    fR.close();
    fN.open(archive_path(o.out, m, 'n'), gz_container(o, 'n'));
    fN.write(names_header(o));
    if (o.use_names) downs[m]->to_file(ctx, b, SCALCE_OUT_NAMES, 0, fN);  // mate 2 repeats mate 1's names (:450-454)
    fN.close();
    if (o.varlen) {  // how long each record really was, in archive order
      OutFile fL;
      fL.open(archive_path(o.out, m, 'l'), gz_container(o, 'l'));
      uint8_t head[scalce_host::LEN_HEADER_BYTES];
      scalce_host::len_header_write(head, p.read_len[m]);
      fL.write(head, sizeof head);
      const std::vector<uint8_t> pad = fetch(ctx, b, SCALCE_OUT_LENGTHS, m);
      const int width = scalce_host::len_entry_width(p.read_len[m]);
      std::vector<uint8_t> entries(pad.size() / 2 * (size_t)width);
      scalce_host::len_entries_write(reinterpret_cast<const uint16_t *>(pad.data()), pad.size() / 2, width, entries.data());
      fL.write(entries);
      fL.close();
    }
  });
  const double t2b = now();
  SCOK(ctx, scalce_batch_finish(b, s_ent));  // the coder is through: sizes of the coded streams, device error word
  const double t2c = now();
  per_mate([&](int m) {
    OutFile fQ;
    fQ.open(archive_path(o.out, m, 'q'), gz_container(o, 'q'));
    fQ.write(qual_header(p.qmap[0].offset));
    if (!no_qual) {  // (-Q / -f: the header and nothing else -- no table (:296), no coder blocks (ac_write of nothing))
      if (!o.no_ac) {
        fQ.write(fetch(ctx, b, SCALCE_OUT_TABLE, m));
        const uint64_t total = N * (uint64_t)p.read_len[m];
        fQ.write(&total, 8);
      }
      downs[m]->qual_to_file(ctx, b, m, fQ);
    }
    fQ.close();
    downs[m].reset();
  });
  const double t2d = now();
  uint64_t new_size = 0;
  for (int m = 0; m < nm; m++)
    for (char ext : {'r', 'q', 'n', 'l'}) {
      struct stat st;
      if (stat(archive_path(o.out, m, ext).c_str(), &st) == 0) new_size += (uint64_t)st.st_size;
    }
  s_ent.release();
  const void *dc = nullptr;
  uint64_t nc = 0;
  SCOK(ctx, scalce_batch_output(b, SCALCE_OUT_BUCKET_COUNTS, 0, &dc, &nc));
  uint64_t unbucketed = 0;
  if (nc >= 8) SCOK(ctx, scalce_memcpy_d2h(ctx, &unbucketed, (const uint8_t *)dc + nc - 8, 8));
  scalce_batch_destroy(b);
  const double t3 = now();
  log_statistics(o, p, N, unbucketed);
  LOG("\tSpill chunks: %u, pieces streamed: %llu\n", st4[3], (unsigned long long)ss.rounds);
  LOG("\tTime elapsed: %.2f s (sample %.2f; stream %.2f = waiting for the reader %.2f + for uploads %.2f + ingest/count/tokenize %.2f; "
      "order %.2f, emit %.2f; reads+names down and written beside the coder %.2f, waiting for the coder %.2f, qualities down and written %.2f, device buffers released %.2f)\n",
      t3 - t0, t1 - t0, ss.total_s - ss.order_s - ss.emit_s, ss.read_wait_s, ss.h2d_wait_s, ss.front_s, ss.order_s, ss.emit_s,
      t2b - t2, t2c - t2b, t2d - t2c, t3 - t2d);
  LOG("\tOriginal size: %.2lfM, new size: %.2lfM, compression factor: %.2lf\n", original / (1024.0 * 1024.0),
      new_size / (1024.0 * 1024.0), new_size ? (double)original / (double)new_size : 0.0);
  return 0;
}

// ---- compress on several GPUs ---------------------------------------------------------------------------------
// One process per GPU (forked before anything touches a GPU), rank r takes the r-th part of the input file, the ranks talk
// RCCL (scalce_sharded_compress) and every rank writes its pieces of the ONE archive with pwrite at the offsets the
// run-wide bucket counts give.  SCALCE_COMM=shm makes all ranks share GPU 0 over the shared-memory rehearsal transport.
static uint64_t count_newlines(int fd, uint64_t a, uint64_t b, int threads) {
  std::atomic<uint64_t> total{0};
  const uint64_t step = 64u << 20;
  std::atomic<uint64_t> next{a};
  auto work = [&]() {
    std::vector<char> buf(8u << 20);
    for (uint64_t at; (at = next.fetch_add(step)) < b;) {
      const uint64_t end = std::min(b, at + step);
      uint64_t n = 0;
      for (uint64_t p = at; p < end;) {
        const ssize_t k = ::pread(fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), end - p), (off_t)p);
        if (k <= 0) FAIL("Read error\n");
        const char *q = buf.data(), *e = q + k;
        while ((q = static_cast<const char *>(memchr(q, '\n', (size_t)(e - q))))) { n++; q++; }
        p += (uint64_t)k;
      }
      total += n;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  return total;
}
// byte offset behind the `skip`-th newline at or after `from`
static uint64_t skip_lines(int fd, uint64_t from, uint64_t size, uint64_t skip) {
  std::vector<char> buf(8u << 20);
  uint64_t p = from;
  while (skip && p < size) {
    const ssize_t k = ::pread(fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), size - p), (off_t)p);
    if (k <= 0) FAIL("Read error\n");
    const char *q = buf.data(), *e = q + k;
    while (skip && (q = static_cast<const char *>(memchr(q, '\n', (size_t)(e - q))))) { skip--; q++; }
    if (!skip) return p + (uint64_t)(q - buf.data());
    p += (uint64_t)k;
  }
  return p;
}
static void pwrite_all(int fd, const void *src, size_t n, uint64_t off) {
  const uint8_t *p = static_cast<const uint8_t *>(src);
  while (n) {
    const ssize_t k = ::pwrite(fd, p, n, (off_t)off);
    if (k <= 0) FAIL("write failed\n");
    p += k; n -= (size_t)k; off += (uint64_t)k;
  }
}
// Bucket k of a stream holds the units of every rank in rank order: amount[r * nb + k] of rank r.  Per bucket: this rank's
// amount, the amount of the ranks before it, and the run's.
struct Shares {
  std::vector<uint64_t> mine, before, all;
  Shares(const uint64_t *amount, uint32_t nb, int world, int rank) : mine(nb, 0), before(nb, 0), all(nb, 0) {
    for (int r = 0; r < world; r++)
      for (uint32_t k = 0; k < nb; k++) {
        const uint64_t a = amount[(size_t)r * nb + k];
        if (r < rank) before[k] += a;
        if (r == rank) mine[k] = a;
        all[k] += a;
      }
  }
};
// This rank's share of a stream that starts at byte `base` of the file, pwritten bucket by bucket at its run-wide place;
// a unit of bucket k is unit(k) bytes.  With `cores` (mate-1 reads) a bucket with units in the run opens with the 12-byte
// header [int32 core][int64 units]: rank 0 (`lead`) writes it, and the rank's own bytes carry one per bucket it has units in.
template <class Unit>
static void place_share(int fd, uint64_t base, const uint8_t *mine, const Shares &sh, Unit unit, const int32_t *cores = nullptr,
                        bool lead = false) {
  const uint64_t h = cores ? 12 : 0;
  for (size_t k = 0; k < sh.all.size(); k++) {
    if (cores && !sh.all[k]) continue;
    if (cores && lead) { uint8_t hd[12]; memcpy(hd, &cores[k], 4); memcpy(hd + 4, &sh.all[k], 8); pwrite_all(fd, hd, 12, base); }
    const uint64_t u = unit(k);
    if (sh.mine[k]) { pwrite_all(fd, mine + h, sh.mine[k] * u, base + h + sh.before[k] * u); mine += h + sh.mine[k] * u; }
    base += h + sh.all[k] * u;
  }
}

static int rank_main(const Options &o, const std::vector<std::string> &files, const char *argv0, int rank, int world, const std::string &tag) {
  const bool shm = getenv("SCALCE_COMM") && !strcmp(getenv("SCALCE_COMM"), "shm");
  const int device = shm ? 0 : rank;
  const int nm = o.paired ? 2 : 1;
  const double t0 = now();
  std::vector<uint8_t> table;
  bool is_text = false;
  scalce_ctx *ctx = open_device(o, argv0, device, table, is_text);
  // communicator
  scalce_comm *comm = nullptr;
  if (shm) {
    if (scalce_comm_create_shm(device, world, rank, ("/scalce_cli_" + tag).c_str(), 1ull << 30, &comm)) FAIL("%s\n", scalce_comm_error(comm));
  } else {
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
  }
  // quality model: the first records of the FILE, the same on every rank (get_quality_stats, compress.cpp:761)
  scalce_params p = params_from(o);
  const std::string path[2] = {files[0], mate_file(files[0], o.paired ? 1 : 0)};
  int fd[2] = {-1, -1};
  uint64_t fsize[2] = {0, 0};
  for (int m = 0; m < nm; m++) {
    if (is_gzip(path[m])) FAIL("--gpus needs plain (not gzip) input: the file is split by byte ranges\n");
    MateSource src;
    src.files.push_back(path[m]);
    quality_model(o, src, m, p, rank == 0);
    fd[m] = ::open(path[m].c_str(), O_RDONLY);
    struct stat st;
    if (fd[m] < 0 || fstat(fd[m], &st) != 0) FAIL("Cannot read file %s\n", path[m].c_str());
    fsize[m] = (uint64_t)st.st_size;
  }
  if (p.read_len[0] <= 0) FAIL("Cannot determine the read length of %s\n", files[0].c_str());
  // ---- this rank's records: line-aligned byte ranges, line counts of everybody, then cuts at multiples of four lines
  Stream s;
  HIPOK(s.create());
  DBuf d_io_buf;
  HIPOK(dbuf_alloc(d_io_buf, sizeof(uint64_t) * (64 + 64 * 4)));
  uint64_t *d_io = d_io_buf.as<uint64_t>();
  uint64_t lo[2], hi[2];
  std::vector<uint64_t> K;  // rank r starts at record K[r], in every mate
  for (int m = 0; m < nm; m++) {
    auto line_start = [&](int r) -> uint64_t {  // first line start at or behind the r-th N-th of the file
      if (r <= 0) return 0;
      if (r >= world) return fsize[m];
      const uint64_t at = fsize[m] / (uint64_t)world * (uint64_t)r;
      return at ? skip_lines(fd[m], at - 1, fsize[m], 1) : 0;
    };
    const uint64_t a = line_start(rank), b = line_start(rank + 1);
    uint64_t mine[2] = {count_newlines(fd[m], a, b, std::max(1, std::min(g_threads, 16))), a};
    std::vector<uint64_t> all((size_t)world * 2);
    HIPOK(hipMemcpy(d_io, mine, sizeof mine, hipMemcpyHostToDevice));
    if (scalce_comm_all_gather(comm, d_io, d_io + 64, sizeof mine, s)) FAIL("%s\n", scalce_comm_error(comm));
    HIPOK(hipStreamSynchronize(s));
    HIPOK(hipMemcpy(all.data(), d_io + 64, all.size() * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> first_line(world + 1, 0);  // run-wide line number at which every tentative range begins
    for (int r = 0; r < world; r++) first_line[r + 1] = first_line[r] + all[2 * r];
    if (first_line[world] % 4) FAIL("%s has %llu lines: not a multiple of 4\n", path[m].c_str(), (unsigned long long)first_line[world]);
    if (m == 1 && first_line[world] != 4 * K[world]) FAIL("mates have different record counts\n");
    // rank r starts at record K_r = ceil(first line of mate 1's r-th range / 4): the same record in every mate
    if (m == 0) { K.assign(world + 1, 0); for (int r = 0; r <= world; r++) K[r] = (first_line[r] + 3) / 4; }
    auto offset_of_line = [&](uint64_t line) -> uint64_t {
      if (line >= first_line[world]) return fsize[m];
      int r = 0;
      while (r + 1 < world && first_line[r + 1] <= line) r++;
      return skip_lines(fd[m], all[2 * r + 1], fsize[m], line - first_line[r]);
    };
    lo[m] = offset_of_line(4 * K[rank]);
    hi[m] = offset_of_line(4 * K[rank + 1]);
  }
  // ---- the piece into HBM
  DBuf d_text_buf[2];
  uint8_t *d_text[2] = {nullptr, nullptr};
  {
    const size_t CH = 256u << 20;
    HBuf pin_buf[2];  // (both go at the end of this block, behind the stream's synchronisation)
    Event ev[2];
    uint8_t *pin[2];
    for (int i = 0; i < 2; i++) { HIPOK(pin_buf[i].alloc(CH)); HIPOK(ev[i].create()); pin[i] = pin_buf[i].as<uint8_t>(); }
    for (int m = 0; m < nm; m++) {
      const uint64_t n = hi[m] - lo[m];
      HIPOK(dbuf_alloc(d_text_buf[m], n + 256));
      d_text[m] = d_text_buf[m].as<uint8_t>();
      uint64_t done = 0;
      for (int i = 0; done < n; i ^= 1) {
        HIPOK(hipEventSynchronize(ev[i]));
        const uint64_t k = std::min<uint64_t>(CH, n - done);
        if (!pread_parallel(fd[m], pin[i], k, lo[m] + done, 16u << 20, g_threads_io())) FAIL("Read error\n");
        HIPOK(hipMemcpyAsync(d_text[m] + done, pin[i], k, hipMemcpyHostToDevice, s));
        HIPOK(hipEventRecord(ev[i], s));
        done += k;
      }
    }
    HIPOK(hipStreamSynchronize(s));
  }
  const double t1 = now();
  // ---- the sharded run
  scalce_batch *b = nullptr;
  const uint64_t rows = (hi[0] - lo[0]) / (2 * (uint64_t)p.read_len[0] + 7) + 64;
  SCOK(ctx, scalce_batch_create(ctx, &p, rows + rows / 3, std::max(hi[0] - lo[0], nm == 2 ? hi[1] - lo[1] : 0) + 256, &b));
  scalce_shard_result res;
  memset(&res, 0, sizeof res);
  if (scalce_sharded_compress(comm, ctx, b, d_text[0], hi[0] - lo[0], nm == 2 ? d_text[1] : nullptr, nm == 2 ? hi[1] - lo[1] : 0, 0, s,
                              nullptr, &res))
    exit(1);
  for (int m = 0; m < nm; m++) d_text_buf[m].release();
  const double t2 = now();
  // ---- every rank writes its pieces of the archive
  const uint32_t nb1 = res.nb1;
  std::vector<int32_t> bucket_pattern(nb1);
  int32_t nst = 0, nbk = 0;
  scalce_patterns_describe_host(table.data(), table.size(), is_text ? 1 : 0, bucket_pattern.data(), nb1, &nst, &nbk);
  const Shares reads(res.counts, nb1, world, rank), names(res.name_bytes, nb1, world, rank);
  std::vector<uint64_t> recsz(nb1);
  const int L0 = p.read_len[0], sz_meta = L0 > 255 ? 2 : 1;
  for (uint32_t k = 0; k < nb1; k++) {
    const int lv = bucket_pattern[k] == SCALCE_ROOT_CORE ? 0 : scalce_pattern_length(ctx, bucket_pattern[k]);
    recsz[k] = (uint64_t)((L0 - lv + 3) / 4 + sz_meta);
  }
  const uint64_t N = res.reads_total;
  const bool lead = rank == 0;  // rank 0 writes the file headers
  auto open_out = [&](int m, char ext, const std::vector<uint8_t> &header) {
    const std::string fn = archive_path(o.out, m, ext);
    if (lead) {
      const int f = ::open(fn.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
      if (f < 0) FAIL("Cannot create %s\n", fn.c_str());
      ::close(f);
    }
    scalce_comm_barrier(comm, s);
    const int f = ::open(fn.c_str(), O_WRONLY);
    if (f < 0) FAIL("Cannot open %s\n", fn.c_str());
    if (lead) pwrite_all(f, header.data(), header.size(), 0);
    return f;
  };
  for (int m = 0; m < nm; m++) {
    const uint64_t L = (uint64_t)p.read_len[m], w = (L + 3) / 4;
    {  // .scalcer: mate 1 in buckets, mate 2 bare rows in mate 1's order
      const std::vector<uint8_t> h = reads_header(o, p.read_len[m]), mine = fetch(ctx, b, SCALCE_OUT_READS, m);
      const int f = open_out(m, 'r', h);
      if (m == 0) place_share(f, h.size(), mine.data(), reads, [&](size_t k) { return recsz[k]; }, bucket_pattern.data(), lead);
      else place_share(f, h.size(), mine.data(), reads, [w](size_t) { return w; });
      ::close(f);
    }
    {  // .scalcen (mate 2 repeats mate 1's names, compress.cpp:450-454)
      const std::vector<uint8_t> h = names_header(o);
      const int f = open_out(m, 'n', h);
      if (o.use_names) place_share(f, h.size(), fetch(ctx, b, SCALCE_OUT_NAMES, 0).data(), names, [](size_t) { return (uint64_t)1; });
      ::close(f);
    }
    {  // .scalceq
      const std::vector<uint8_t> h = qual_header(p.qmap[0].offset);
      const int f = open_out(m, 'q', h);
      if (!o.no_ac) {  // the table and the symbol count, then the coded blocks of every rank in rank order
        if (lead) {
          const std::vector<uint8_t> tb = fetch(ctx, b, SCALCE_OUT_TABLE, m);
          pwrite_all(f, tb.data(), tb.size(), h.size());
          const uint64_t total = N * L;
          pwrite_all(f, &total, 8, h.size() + tb.size());
        }
        uint64_t before = 0;
        for (int r = 0; r < rank; r++) before += res.coded_bytes[m][r];
        const std::vector<uint8_t> mine = fetch(ctx, b, SCALCE_OUT_QUAL, m);
        pwrite_all(f, mine.data(), mine.size(), h.size() + QTABLE_WORDS * 4 + 8 + before);
      } else {  // -A: the raw q' rows, bucket by bucket in rank order (compress.cpp:389-390)
        place_share(f, h.size(), fetch(ctx, b, SCALCE_OUT_QSTREAM, m).data(), reads, [L](size_t) { return L; });
      }
      ::close(f);
    }
  }
  scalce_comm_barrier(comm, s);
  const double t3 = now();
  if (lead) {
    LOG("\tDone with file %s, %llu reads found\n", files[0].c_str(), (unsigned long long)N);
    log_statistics(o, p, N, reads.all[nb1 - 1]);
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
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) FAIL("Cannot read %s\n", path.c_str());
  OutFile out;
  out.open(path + ".gz.tmp", true);
  std::vector<uint8_t> buf(256u << 20);
  for (;;) {
    const ssize_t k = ::read(fd, buf.data(), buf.size());
    if (k < 0) FAIL("Read error on %s\n", path.c_str());
    if (k == 0) break;
    out.write(buf.data(), (size_t)k);
  }
  ::close(fd);
  out.close();
  if (rename((path + ".gz.tmp").c_str(), path.c_str()) != 0) FAIL("Cannot replace %s\n", path.c_str());
}

static int multi_gpu_compress(const Options &o_in, const std::vector<std::string> &files_in, const char *argv0) {
  if (o_in.gpus > 64) FAIL("--gpus: at most 64\n");
  LOG("Preprocessing FASTQ files ...\n");
  const std::string tag = std::to_string(getpid()) + "_" + std::to_string((long)time(nullptr));
  set_threads(o_in, 1);
  Options o = o_in;
  o.container = 0;  // the ranks write plain; -c gz is applied to the finished files below
  std::vector<std::string> files = files_in;
  if (!plain_single_input(o, files)) {
    const double t0 = now();
    files.assign(1, materialize_inputs(o, files_in, tag));
    LOG("\t%zu input file(s) per mate written out as one plain file under %s (%.2f s)\n", files_in.size(), o.temp.c_str(), now() - t0);
  }
  set_threads(o, o.gpus);  // (the ranks share the host)
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
    for (int m = 0; m < (o.paired ? 2 : 1); m++)
      for (char ext : {'r', 'n', 'q'}) unlink(archive_path(o.out, m, ext).c_str());
    fprintf(stderr, "(ERROR) a rank failed\n");
    return 1;
  }
  if (o_in.container != 0) {
    set_threads(o_in, 1);
    const double t0 = now();
    for (int m = 0; m < (o.paired ? 2 : 1); m++)
      for (char ext : {'r', 'n', 'q'})
        if (gz_container(o_in, ext)) gzip_in_place(archive_path(o.out, m, ext));
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
// one file of the archive behind scalce_read_fn: a gzip container through the parallel reader, which streams (no seek), or
// a plain file through pread
struct ArchiveFile {
  std::string path;
  bool gz = false;
  scalce_host::ParGz z;
  int fd = -1;
  uint64_t off = 0;
  void open(const std::string &p) {
    path = p;
    gz = is_gzip(p);  // container sniffing (decompress.cpp:99-113)
    if (gz) { if (!z.open(p, g_threads_gz())) FAIL("Cannot read file %s\n", p.c_str()); }
    else if ((fd = ::open(p.c_str(), O_RDONLY)) < 0) FAIL("Cannot read file %s\n", p.c_str());
  }
  static int64_t read(void *user, void *dst, uint64_t cap) {
    ArchiveFile *f = static_cast<ArchiveFile *>(user);
    if (f->gz) return f->z.read(dst, cap);
    const ssize_t k = ::pread(f->fd, dst, (size_t)std::min<uint64_t>(cap, 1u << 30), (off_t)f->off);
    if (k > 0) f->off += (uint64_t)k;
    return (int64_t)k;
  }
  // scalce_skip_fn of a plain file: the offset moves, up to the file's end
  static int64_t skip(void *user, uint64_t nbytes) {
    ArchiveFile *f = static_cast<ArchiveFile *>(user);
    struct stat st;
    if (f->gz || fstat(f->fd, &st) != 0) return -1;
    const uint64_t size = (uint64_t)st.st_size, k = std::min(nbytes, size > f->off ? size - f->off : 0);
    f->off += k;
    return (int64_t)k;
  }
  ~ArchiveFile() { if (fd >= 0) ::close(fd); }
};

// the text of the windows, as they arrive, into OUT_<m>.fastq -- or, with -S n, into a new part every n records (pairs
// under -i; decompress.cpp:276-287), cut at the window's record offsets, across window boundaries
struct TextSink {
  const Options *o = nullptr;
  struct PerMate {
    OutFile f;
    bool open = false;
    int part = 0;
    uint64_t in_part = 0, files = 0;
    char fn[4096];
  } pm[2];
  void open_next(int m) {
    PerMate &x = pm[m];
    x.part++;
    if (o->out == "-") snprintf(x.fn, sizeof x.fn, "-");
    else if (o->split) snprintf(x.fn, sizeof x.fn, "%s.%d_%d.fastq", o->out.c_str(), x.part, m + 1);
    else snprintf(x.fn, sizeof x.fn, "%s_%d.fastq", o->out.c_str(), m + 1);
    x.f.open(x.fn, false);
    x.open = true;
    x.in_part = 0;
    x.files++;
  }
  void close_part(int m) {
    PerMate &x = pm[m];
    if (x.f.f == stdout) fflush(stdout);
    x.f.close();
    x.open = false;
    LOG("Created %s with %lld %s\n", x.fn, (long long)x.in_part, o->interleave ? "pairs" : "reads");
  }
  static int write(void *user, int m, uint64_t, uint64_t nrec, const void *text, uint64_t nbytes, const uint64_t *roff) {
    TextSink *t = static_cast<TextSink *>(user);
    PerMate &x = t->pm[m];
    const uint8_t *b = static_cast<const uint8_t *>(text);
    if (!t->o->split) {
      if (!x.open) t->open_next(m);
      x.f.write(b, nbytes);
      x.in_part += nrec;
      if (x.f.f == stdout) fflush(stdout);  // -o -: a window is out when it has arrived
      return 0;
    }
    for (uint64_t k = 0; k < nrec;) {
      if (!x.open) t->open_next(m);
      const uint64_t take = std::min<uint64_t>((uint64_t)t->o->split - x.in_part, nrec - k);
      x.f.write(b + roff[k], roff[k + take] - roff[k]);
      x.in_part += take;
      k += take;
      if (x.in_part == (uint64_t)t->o->split) t->close_part(m);
    }
    return 0;
  }
  void finish(int m) {  // (an archive without records still gives its one empty file)
    if (!pm[m].open && !pm[m].files) open_next(m);
    if (pm[m].open) close_part(m);
  }
};

// One path for every archive: scalce_stream_decompress moves it through the device in windows of whole records.  The read
// callbacks hand out the files as they are read, the write callback writes each window's text as it arrives.
static int do_decompress(const Options &o, const std::string &path, scalce_ctx *ctx) {
  const double t0 = now();
  const int nm = o.pairs() ? 2 : 1;
  std::string base[2] = {path, path};
  if (o.pairs() && !second_file(path, base[1])) FAIL("Cannot get file name for paired end for file %s.\n", path.c_str());
  // a variable-length archive has a length stream next to the other three: without the file, the reads come back padded
  bool has_lens[2] = {false, false};
  for (int m = 0; m < nm; m++) {
    const std::string lpath = scalce_name(base[m], 'l');
    struct stat lst;
    if (stat(lpath.c_str(), &lst) != 0) continue;
    if (o.interleave) FAIL("%s: an archive of variable-length reads is decompressed mate by mate (-r), not interleaved (-i)\n", lpath.c_str());
    if (o.fasta || o.no_qual) FAIL("%s: an archive of variable-length reads is decompressed with its qualities, not with -Q / -f\n", lpath.c_str());
    has_lens[m] = true;
  }
  ArchiveFile files[2][3], lens[2];
  scalce_read_fn rd[2][3];
  void *user[2][3];
  static const char ext[3] = {'r', 'n', 'q'};
  for (int m = 0; m < 2; m++)
    for (int k = 0; k < 3; k++) {
      rd[m][k] = m < nm ? ArchiveFile::read : nullptr;
      user[m][k] = &files[m][k];
      if (m < nm) files[m][k].open(scalce_name(base[m], ext[k]));
    }
  scalce_unpack_params p;
  memset(&p, 0, sizeof p);
  for (int m = 0; m < nm; m++) {
    if (!has_lens[m]) continue;
    lens[m].open(scalce_name(base[m], 'l'));
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
  TextSink sink;
  sink.o = &o;
  scalce_unpack_range rg;
  memset(&rg, 0, sizeof rg);
  rg.first_record = o.range_first;
  rg.nrecords = o.range_count;
  for (int m = 0; m < nm; m++)
    for (int k = 0; k < 3; k++) rg.skip[m][k] = files[m][k].gz ? nullptr : ArchiveFile::skip;
  scalce_unpack_stats st;
  scalce_unpack_range_stats rs;
  char err[1024] = "";
  const int rc = scalce_stream_decompress_range(ctx, &p, &rg, rd, user, TextSink::write, &sink, &st, &rs, err, sizeof err);
  if (rc) {
    // (parts already written stay where they are)
    if (st.error_wants_file && st.error_mate >= 0 && st.error_stream >= 0)
      FAIL("%s %s\n", st.error_stream == 0 ? base[st.error_mate].c_str() : files[st.error_mate][st.error_stream].path.c_str(), err);
    fprintf(stderr, "%s%s\n", strncmp(err, "(ERROR)", 7) ? "(ERROR) " : "", err);
    exit(1);
  }
  for (int m = 0; m < (o.interleave ? 1 : nm); m++) sink.finish(m);
  LOG("\tTime elapsed: %.2f s (archive files read %.2f; qualities up and decoded %.2f; records to text %.2f; text down and written %.2f%s)\n",
      now() - t0, st.read_wait_s, st.decode_s, st.records_s, st.write_s, nm == 2 && !o.interleave ? ", one mate after the other" : "");
  LOG("\tWindows: %llu of up to %llu bytes of text; device memory held at most %llu bytes\n", (unsigned long long)st.windows,
      (unsigned long long)st.window_text_bytes, (unsigned long long)st.peak_device_bytes);
  if (o.has_range) {
    char total[32] = "unknown";
    if (rs.total_records != ~0ull) snprintf(total, sizeof total, "%llu", (unsigned long long)rs.total_records);
    LOG("\tRange: records %llu to %llu of %s; quality frames decoded %llu, passed over %llu\n", (unsigned long long)rs.first_record,
        (unsigned long long)(rs.first_record + rs.nrecords), total, (unsigned long long)(rs.frames_decoded[0] + rs.frames_decoded[1]),
        (unsigned long long)(rs.frames_passed[0] + rs.frames_passed[1]));
  }
  return 0;
}

int main(int argc, char **argv) {
  const double t_main = now();
  Options o;
  LOG("SCALCE %s [MI355X / HIP]\n", SCALCE_VERSION);
  static struct option long_opt[] = {{"help", 0, 0, 'h'}, {"lossy-percentage", 1, 0, 'p'}, {"decompress", 0, 0, 'd'},
                                     {"compression", 1, 0, 'c'}, {"output", 1, 0, 'o'}, {"sample-size", 1, 0, 's'},
                                     {"no-qualities", 0, 0, 'Q'}, {"patterns", 1, 0, 'P'}, {"temp-directory", 1, 0, 't'},
                                     {"bucket-set-size", 1, 0, 'B'}, {"paired-end", 0, 0, 'r'}, {"skip-names", 1, 0, 'n'},
                                     {"split-reads", 1, 0, 'S'}, {"fasta", 0, 0, 'f'}, {"threads", 1, 0, 'T'},
                                     {"version", 0, 0, 'v'}, {"no-arithmetic", 0, 0, 'A'}, {"patterns-bin", 1, 0, 1000},
                                     {"gpus", 1, 0, 1001}, {"interleave", 0, 0, 'i'}, {"window", 1, 0, 1002},
                                     {"records", 1, 0, 1003}, {"variable-length", 0, 0, 1004},
                                     {"max-length", 1, 0, 1005}, {0, 0, 0, 0}};
  int opt;
  while ((opt = getopt_long(argc, argv, "vhp:T:dc:o:fs:t:B:rQAn:P:S:i", long_opt, 0)) != -1) {
    switch (opt) {
      case 'v': return 0;
      case 'h': fputs(HELP_TEXT, stdout); return 0;
      case 'A': o.no_ac = true; break;
      case 'f': o.fasta = true; break;
      case 'Q': o.no_qual = true; break;
      case 'c':
        if (!strcmp(optarg, "gz") || !strcmp(optarg, "pigz")) o.container = 1;
        else if (!strcmp(optarg, "no")) o.container = 0;
        else if (!strcmp(optarg, "bz")) FAIL("bzip2 containers are outside this build's scope (SURVEY.md section 2, #18: host-side container code); use gz or no\n");
        else FAIL("Unknown compression mode. See help for details.\n");
        break;
      case 'B': {
        std::string s = optarg;
        const char al = s.empty() ? 0 : s.back();
        uint64_t unit = 1024 * 1024ull;
        if (al == 'G') unit *= 1024; else if (al != 'M') FAIL("Size parameter must be ended with G or M.\n");
        s.pop_back();
        o.bucket_set_size = unit * (uint64_t)atoi(s.c_str());
      } break;
      case 'p': o.lossy = atoi(optarg); break;
      case 'T': o.threads = atoi(optarg); break;
      case 'S': o.split = atoi(optarg); break;
      case 'r': o.paired = true; break;
      case 'i': o.interleave = true; break;
      case 's': o.sample = atoi(optarg); break;
      case 'd': o.decompress = true; break;
      case 'P': o.patterns = optarg; break;
      case 't': o.temp = optarg; break;
      case 'o': o.out = optarg; break;
      case 'n': o.use_names = false; o.library = optarg; break;
      case 1000: o.patterns_bin = optarg; break;
      case 1001: o.gpus = atoi(optarg); break;
      case 1002: {
        char *e = nullptr;
        const unsigned long long v = strtoull(optarg, &e, 10);
        const uint64_t unit = *e == 'K' ? 1ull << 10 : *e == 'M' ? 1ull << 20 : *e == 'G' ? 1ull << 30 : 1;
        if (e == optarg || !v || (*e && (unit == 1 || e[1]))) FAIL("--window takes a positive number of bytes, optionally ended with K, M or G.\n");
        o.window = v * unit;
      } break;
      case 1003: {
        // FIRST[:COUNT], both plain decimal numbers (strtoull alone would take a sign, blanks and an empty string)
        auto number = [](const char *b, const char *e, uint64_t &v) {
          if (b == e || e - b > 19) return false;
          v = 0;
          for (; b != e; b++) { if (*b < '0' || *b > '9') return false; v = v * 10 + (uint64_t)(*b - '0'); }
          return true;
        };
        const char *colon = strchr(optarg, ':'), *end = optarg + strlen(optarg);
        if (!number(optarg, colon ? colon : end, o.range_first) || (colon && !number(colon + 1, end, o.range_count)))
          FAIL("--records takes FIRST or FIRST:COUNT, two non-negative numbers of records.\n");
        o.has_range = true;
      } break;
      case 1004: o.varlen = true; break;
      case 1005:
        o.max_length = atoi(optarg);
        if (o.max_length < 1 || o.max_length > 2498) FAIL("--max-length takes the longest read's number of bases, 1 to 2498.\n");
        o.varlen = true;
        break;
      default: fputs(HELP_TEXT, stdout); return 0;
    }
  }
  std::vector<std::string> files(argv + optind, argv + argc);
  // check_arguments, main.cpp:120-164
  if (o.interleave && o.paired) FAIL("Interleaved option (-i) cannot be used with paired-end option (-r).\n");
  if (o.out.empty()) FAIL("No output file specified.\n");
  if (!o.use_names && o.library.empty()) FAIL("No library name specified.\n");
  if (o.has_range && !o.decompress) FAIL("--records can be only used with decompression (-d).\n");
  if (o.decompress && files.size() > 1) FAIL("Too many files specified (decompression only supports one file).\n");
  if (o.lossy < 0 || o.lossy > 100) FAIL("Percentage must be in range [0,100].\n");
  if (o.out == "-" && (o.split || o.paired)) FAIL("stdout can be only used with single-end file decompression. It cannot be used with --split-reads option!\n");
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
  if (o.gpus > 1 && !o.decompress) {  // forks before anything touches a GPU
    // (a run that -B does not cut anywhere is one chunk: scalce_sharded_compress sends all its rows to rank 0)
    return multi_gpu_compress(o, files, argv[0]);
  }
  std::vector<uint8_t> table;
  bool is_text = false;
  scalce_ctx *ctx = open_device(o, argv[0], 0, table, is_text);
  set_threads(o, 1);
  const double t_ready = now();
  const int rc = o.decompress ? do_decompress(o, files[0], ctx) : do_compress(o, files, ctx);
  scalce_ctx_destroy(ctx);
  LOG("\tProcess: device and core table ready %.2f s after main() began, %.2f s in all\n", t_ready - t_main, now() - t_main);
  LOG("Done!\n");
  return rc;
}
