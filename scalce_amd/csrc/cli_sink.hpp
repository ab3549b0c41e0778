// cli_sink.hpp -- the two ends of `scalce -d` on the host: an archive file behind the library's read and skip callbacks,
// and the FASTQ text of the windows into its output files.  Host code only: of scalce_hip.h it uses the callback types.
#pragma once
#include "../../include/scalce_hip.h"
#include "cli_io.hpp"

// one file of the archive behind scalce_read_fn: a gzip container through the parallel reader, which streams (no seek), or
// a plain file through pread
struct ArchiveFile {
  std::string path;
  bool gz = false;
  scalce_host::ParGz z;
  Fd fd;
  uint64_t off = 0;
  void open(const std::string &p) {
    path = p;
    gz = is_gzip(p);  // container sniffing (decompress.cpp:99-113)
    if (gz) { if (!z.open(p, g_threads_gz())) FAIL("Cannot read file %s\n", p.c_str()); }
    else if (!fd.open(p, O_RDONLY)) FAIL("Cannot read file %s\n", p.c_str());
  }
  static int64_t read(void *user, void *dst, uint64_t cap) {
    ArchiveFile *f = static_cast<ArchiveFile *>(user);
    if (f->gz) return f->z.read(dst, cap);
    const ssize_t k = ::pread(f->fd.get(), dst, (size_t)std::min<uint64_t>(cap, 1u << 30), (off_t)f->off);
    if (k > 0) f->off += (uint64_t)k;
    return (int64_t)k;
  }
  // scalce_skip_fn of a plain file: the offset moves, up to the file's end
  static int64_t skip(void *user, uint64_t nbytes) {
    ArchiveFile *f = static_cast<ArchiveFile *>(user);
    struct stat st;
    if (f->gz || fstat(f->fd.get(), &st) != 0) return -1;
    const uint64_t size = (uint64_t)st.st_size, k = std::min(nbytes, size > f->off ? size - f->off : 0);
    f->off += k;
    return (int64_t)k;
  }
};

// the text of the windows, as they arrive, into OUT_<m>.fastq -- or, with -S n, into a new part every n records (pairs
// under -i; decompress.cpp:276-287), cut at the window's record offsets, across window boundaries
struct TextSink {
  std::string out;          // -o
  int split = 0;            // -S
  bool interleave = false;  // -i: a part counts pairs
  bool discard = false;     // --test: the text is dropped, no file is made
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
    if (out == "-") snprintf(x.fn, sizeof x.fn, "-");
    else if (split) snprintf(x.fn, sizeof x.fn, "%s.%d_%d.fastq", out.c_str(), x.part, m + 1);
    else snprintf(x.fn, sizeof x.fn, "%s_%d.fastq", out.c_str(), m + 1);
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
    LOG("Created %s with %lld %s\n", x.fn, (long long)x.in_part, interleave ? "pairs" : "reads");
  }
  static int write(void *user, int m, uint64_t, uint64_t nrec, const void *text, uint64_t nbytes, const uint64_t *roff) {
    TextSink *t = static_cast<TextSink *>(user);
    if (t->discard) return 0;
    PerMate &x = t->pm[m];
    const uint8_t *b = static_cast<const uint8_t *>(text);
    if (!t->split) {
      if (!x.open) t->open_next(m);
      x.f.write(b, nbytes);
      x.in_part += nrec;
      if (x.f.f == stdout) fflush(stdout);  // -o -: a window is out when it has arrived
      return 0;
    }
    for (uint64_t k = 0; k < nrec;) {
      if (!x.open) t->open_next(m);
      const uint64_t take = std::min<uint64_t>((uint64_t)t->split - x.in_part, nrec - k);
      x.f.write(b + roff[k], roff[k + take] - roff[k]);
      x.in_part += take;
      k += take;
      if (x.in_part == (uint64_t)t->split) t->close_part(m);
    }
    return 0;
  }
  void finish(int m) {  // (an archive without records still gives its one empty file)
    if (discard) return;
    if (!pm[m].open && !pm[m].files) open_next(m);
    if (pm[m].open) close_part(m);
  }
};
