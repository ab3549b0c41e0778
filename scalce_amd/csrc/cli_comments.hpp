// cli_comments.hpp -- what the `scalce` tool does on the host for --keep-comments: the header of a PREFIX_<m>.scalcec file, the
// line of the log, and whether -d finds such a file next to an archive.  Host code only: no HIP, nothing of the library.
#pragma once
#include <sys/stat.h>

#include <string>

#include "cli_io.hpp"
#include "commentstream.hpp"

// the 24 header bytes of a comment stream (commentstream.hpp) into its file, in front of the entries
inline void comment_file_header(OutFile &f, uint32_t longest, uint64_t records) {
  uint8_t head[scalce_host::COMMENT_HEADER_BYTES];
  scalce_host::comment_header_write(head, longest, records);
  f.write(head, sizeof head);
}
// per mate: how many entries, their bytes in the stream (newlines included), the longest
inline void comment_log(uint64_t records, uint64_t bytes, uint32_t longest) {
  LOG("\tComments: %llu records, %llu bytes, longest %u\n", (unsigned long long)records, (unsigned long long)bytes, longest);
}
inline bool comment_file_present(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}
