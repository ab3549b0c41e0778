// cli_exceptions.hpp -- what the `scalce` tool does on the host for --keep-bases: the header of a PREFIX_<m>.scalcex file, the
// line of the log, and whether -d finds such a file next to an archive.  Host code only: no HIP, nothing of the library.
#pragma once
#include <sys/stat.h>

#include <string>

#include "cli_io.hpp"
#include "exceptionstream.hpp"

// the 32 header bytes of an exception stream (exceptionstream.hpp) into its file, in front of the entries
inline void exception_file_header(OutFile &f, uint32_t read_len, uint64_t records, uint64_t entries) {
  uint8_t head[scalce_host::EXCEPTION_HEADER_BYTES];
  scalce_host::exception_header_write(head, read_len, records, entries);
  f.write(head, sizeof head);
}
// per mate: how many entries, in how many of the records
inline void exception_log(uint64_t records, uint64_t entries, uint64_t records_with_one) {
  LOG("\tBases: %llu exceptions in %llu of %llu records\n", (unsigned long long)entries, (unsigned long long)records_with_one,
      (unsigned long long)records);
}
inline bool exception_file_present(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}
