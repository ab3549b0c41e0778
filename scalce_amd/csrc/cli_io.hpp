// cli_io.hpp -- what the `scalce` tool does with files on the host: messages, thread counts, owned descriptors, parallel
// reads, line counting and the plain / gzip output file.  Host code only: no HIP, nothing of the library.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "pargz.hpp"

inline void LOG(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
}
[[noreturn]] inline void FAIL(const char *fmt, ...) {  // ERROR(), const.h:77-81
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "(ERROR) ");
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  exit(1);
}
inline double now() {
  struct timeval t;
  gettimeofday(&t, 0);
  return t.tv_sec + 1e-6 * t.tv_usec;
}

// Host threads: `asked` (-T), else the cores shared by `procs` processes (a process alone leaves one to its main thread), at
// most 64.  Plain files are read by up to 8 of them, gzip members inflated by up to 32, the gz containers deflated by all.
inline int g_threads = 1;
inline void set_threads(int asked, int procs) {
  const int hw = (int)std::thread::hardware_concurrency();
  g_threads = asked > 0 ? asked : std::max(1, std::min(64, procs > 1 ? hw / procs : hw - 1));
}
inline int g_threads_io() { return std::max(1, std::min(g_threads, 8)); }
inline int g_threads_gz() { return std::max(1, std::min(g_threads, 32)); }

// A file descriptor that closes itself: move-only, the shape of hip_own.hpp's handles.
struct Fd {
  int fd = -1;
  Fd() = default;
  Fd(Fd &&o) noexcept : fd(o.fd) { o.fd = -1; }
  Fd &operator=(Fd &&o) noexcept { if (this != &o) { release(); fd = o.fd; o.fd = -1; } return *this; }
  ~Fd() { release(); }
  bool open(const std::string &path, int flags, mode_t mode = 0) { release(); fd = ::open(path.c_str(), flags, mode); return fd >= 0; }
  void release() { if (fd >= 0) ::close(fd); fd = -1; }
  int get() const { return fd; }
};
static_assert(!std::is_copy_constructible<Fd>::value && !std::is_copy_assignable<Fd>::value, "an Fd is handed over with std::move");

inline bool is_gzip(const std::string &path) {  // the gzip magic (the reference's readers sniff it too, decompress.cpp:99-113)
  Fd f;
  uint8_t mg[2] = {0, 0};
  return f.open(path, O_RDONLY) && ::pread(f.get(), mg, 2, 0) == 2 && mg[0] == 0x1F && mg[1] == 0x8B;
}
// fn(a, b) on the slices [a, b) of [0, n), `slice` bytes each, taken in turn by up to `threads` threads (the caller's included)
template <class Fn> void for_slices(uint64_t n, uint64_t slice, int threads, Fn fn) {
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
inline bool pread_parallel(int fd, uint8_t *dst, uint64_t n, uint64_t off, uint64_t slice, int threads) {
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
inline std::vector<uint8_t> read_whole(const std::string &path) {
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
  Fd f;
  struct stat st;
  if (!f.open(path, O_RDONLY) || fstat(f.get(), &st) != 0) FAIL("Cannot read file %s\n", path.c_str());
  out.resize((size_t)st.st_size);
  if (!pread_parallel(f.get(), out.data(), out.size(), 0, 64u << 20, g_threads_io())) FAIL("Read error on %s\n", path.c_str());
  return out;
}
inline bool second_file(const std::string &p, std::string &out) {  // get_second_file, const.cpp:51-64
  out = p;
  for (int i = (int)out.size() - 1; i >= 0; i--)
    if (out[i] == '1') { out[i] = '2'; return true; }
  return false;
}
inline std::string mate_file(const std::string &f, int m) {  // input f's file of mate m
  std::string out = f;
  if (m && !second_file(f, out)) FAIL("Cannot get file name for paired end for file %s. File should contain character 1.\n", f.c_str());
  return out;
}
inline void pwrite_all(int fd, const void *src, size_t n, uint64_t off) {
  const uint8_t *p = static_cast<const uint8_t *>(src);
  while (n) {
    const ssize_t k = ::pwrite(fd, p, n, (off_t)off);
    if (k <= 0) FAIL("write failed\n");
    p += k; n -= (size_t)k; off += (uint64_t)k;
  }
}

// newlines in bytes [a, b) of fd, counted in slices of 64 MiB by up to `threads` threads
inline uint64_t count_newlines(int fd, uint64_t a, uint64_t b, int threads) {
  std::atomic<uint64_t> total{0};
  for_slices(b > a ? b - a : 0, 64u << 20, threads, [&](uint64_t sa, uint64_t sb) {
    std::unique_ptr<char[]> buf(new char[8u << 20]);
    uint64_t n = 0;
    for (uint64_t p = a + sa, end = a + sb; p < end;) {
      const ssize_t k = ::pread(fd, buf.get(), (size_t)std::min<uint64_t>(8u << 20, end - p), (off_t)p);
      if (k <= 0) FAIL("Read error\n");
      const char *q = buf.get(), *e = q + k;
      while ((q = static_cast<const char *>(memchr(q, '\n', (size_t)(e - q))))) { n++; q++; }
      p += (uint64_t)k;
    }
    total += n;
  });
  return total;
}
// byte offset behind the `skip`-th newline at or after `from`
inline uint64_t skip_lines(int fd, uint64_t from, uint64_t size, uint64_t skip) {
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
