// cli_input.hpp -- one mate's input as the `scalce` tool reads it: the files of the command line joined into one record
// stream, and the quality sample taken from its first records.  Host code only.
#pragma once
#include "cli_io.hpp"

// One mate's input: the files of the command line one after the other (compress.cpp:756-797 runs them through the same
// trie; the record stream is their concatenation), each plain or gzip (the reference opens everything through zlib,
// :767-779).  Plain files are read by parallel pread straight into the pinned chunk the streaming host hands in.
struct MateSource {
  std::vector<std::string> files;
  size_t cur = 0;
  Fd fd;                      // the plain file being read
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
    if (!fd.open(path, O_RDONLY)) FAIL("Cannot read file %s\n", path.c_str());
#ifdef POSIX_FADV_SEQUENTIAL
    posix_fadvise(fd.get(), 0, 0, POSIX_FADV_SEQUENTIAL);
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
      if (fd.get() < 0 && !gz) {
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
      if (gz) { pgz.close(); gz = false; } else fd.release();
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
    if (fstat(fd.get(), &st) != 0) return -1;
    const uint64_t want = std::min(cap, (uint64_t)st.st_size > fpos ? (uint64_t)st.st_size - fpos : 0);
    if (!pread_parallel(fd.get(), dst, want, fpos, 16u << 20, g_threads_io())) return -1;
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
inline void sample_stats(const uint8_t *t, size_t n, int sample, int32_t stat[128], int &read_length, int stride = 1, int first = 0) {
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
