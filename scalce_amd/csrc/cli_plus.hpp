// cli_plus.hpp -- what the `scalce` tool does on the host for --keep-plus: the header of a PREFIX_<m>.scalcep file, the line of
// the log, and whether -d finds such a file next to an archive.  Host code only: no HIP, nothing of the library.
#pragma once
#include <sys/stat.h>

#include <string>

#include "cli_io.hpp"
#include "plusstream.hpp"

// the 24 header bytes of a plus-line stream (plusstream.hpp) into its file, in front of the entries
inline void plus_file_header(OutFile &f, uint32_t longest, uint64_t records) {
  uint8_t head[scalce_host::PLUS_HEADER_BYTES];
  scalce_host::plus_header_write(head, longest, records);
  f.write(head, sizeof head);
}
// per mate: how many entries, how many of them repeat the header line or hold a line of their own, the longest stored entry
inline void plus_log(uint64_t records, uint64_t repeats, uint64_t literals, uint32_t longest) {
  LOG("\tPlus lines: %llu records, %llu repeated, %llu literal, longest %u\n", (unsigned long long)records, (unsigned long long)repeats,
      (unsigned long long)literals, longest);
}
inline bool plus_file_present(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}
