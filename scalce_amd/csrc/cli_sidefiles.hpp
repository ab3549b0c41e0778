// cli_sidefiles.hpp -- what the `scalce` tool does on the host for the side files of an archive (.scalcel, .scalceo, .scalcec,
// .scalcex, .scalcep): the header of such a file, the line of the log of --keep-comments, --keep-plus and --keep-bases, and
// whether -d finds such a file next to an archive.  Host code only: no HIP, nothing of the library.
#pragma once
#include <sys/stat.h>

#include <string>

#include "cli_io.hpp"
#include "commentstream.hpp"
#include "exceptionstream.hpp"
#include "lenstream.hpp"
#include "orderstream.hpp"
#include "plusstream.hpp"

// the N header bytes of a side stream, as its *_header_write(head, fields...) makes them, into its file in front of the entries
template <size_t N, class Write, class... Fields> void side_file_header(OutFile &f, Write write, Fields... fields) {
  uint8_t head[N];
  write(head, fields...);
  f.write(head, N);
}
inline bool side_file_present(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}
// per mate: how many entries, their bytes in the stream (newlines included), the longest
inline void comment_log(uint64_t records, uint64_t bytes, uint32_t longest) {
  LOG("\tComments: %llu records, %llu bytes, longest %u\n", (unsigned long long)records, (unsigned long long)bytes, longest);
}
// per mate: how many entries, how many of them repeat the header line or hold a line of their own, the longest stored entry
inline void plus_log(uint64_t records, uint64_t repeats, uint64_t literals, uint32_t longest) {
  LOG("\tPlus lines: %llu records, %llu repeated, %llu literal, longest %u\n", (unsigned long long)records, (unsigned long long)repeats,
      (unsigned long long)literals, longest);
}
// per mate: how many entries, in how many of the records
inline void exception_log(uint64_t records, uint64_t entries, uint64_t records_with_one) {
  LOG("\tBases: %llu exceptions in %llu of %llu records\n", (unsigned long long)entries, (unsigned long long)records_with_one,
      (unsigned long long)records);
}
