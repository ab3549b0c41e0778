// cli_shares.hpp -- the arithmetic of a --gpus run that decides bytes of the archive: which records of the input a rank
// takes, and where its share of every bucket is written.  Host code only; the ranks' numbers come in as plain arrays.
#pragma once
#include "cli_io.hpp"

// ---- record cuts ------------------------------------------------------------------------------------------
// Rank r first takes the tentative range of lines that begin in the r-th world-th of the file's bytes; the ranks then
// exchange how many lines each found, and the ranges are moved to multiples of four lines.

// first line start at or behind the r-th world-th of the file (rank r's tentative range begins there)
inline uint64_t line_start(int fd, uint64_t size, int world, int r) {
  if (r <= 0) return 0;
  if (r >= world) return size;
  const uint64_t at = size / (uint64_t)world * (uint64_t)r;
  return at ? skip_lines(fd, at - 1, size, 1) : 0;
}
// One mate's tentative ranges as every rank sees them after the exchange: gathered[2 r] = lines of rank r's range,
// gathered[2 r + 1] = the byte offset at which it begins.
struct LineRanges {
  enum Refusal { OK, NOT_WHOLE_RECORDS, MATES_DIFFER };
  int world;
  std::vector<uint64_t> first_line, start;  // run-wide line number (world + 1 of them) and byte offset at which range r begins
  LineRanges(int world_, const uint64_t *gathered) : world(world_), first_line(world_ + 1, 0), start(world_, 0) {
    for (int r = 0; r < world; r++) { first_line[r + 1] = first_line[r] + gathered[2 * r]; start[r] = gathered[2 * r + 1]; }
  }
  uint64_t lines() const { return first_line[world]; }
  // rank r starts at record K[r] = ceil(first line of mate 1's r-th range / 4): the same record in every mate
  std::vector<uint64_t> first_records() const {
    std::vector<uint64_t> K(world + 1);
    for (int r = 0; r <= world; r++) K[r] = (first_line[r] + 3) / 4;
    return K;
  }
  // why the run cannot go on; K: mate 1's first_records() when this is mate 2, else nullptr
  Refusal refusal(const std::vector<uint64_t> *K) const {
    if (lines() % 4) return NOT_WHOLE_RECORDS;
    if (K && lines() != 4 * (*K)[world]) return MATES_DIFFER;
    return OK;
  }
  // byte offset at which the run-wide line `line` begins (the file's size behind its last line)
  uint64_t offset_of_line(int fd, uint64_t size, uint64_t line) const {
    if (line >= lines()) return size;
    int r = 0;
    while (r + 1 < world && first_line[r + 1] <= line) r++;
    return skip_lines(fd, start[r], size, line - first_line[r]);
  }
};

// ---- placement ------------------------------------------------------------------------------------------
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
void place_share(int fd, uint64_t base, const uint8_t *mine, const Shares &sh, Unit unit, const int32_t *cores = nullptr,
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
