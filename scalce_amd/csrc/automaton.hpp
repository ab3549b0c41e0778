// automaton.hpp -- host-side core table: patterns.bin / text list -> BFS-ordered DFA.
// Replaces read_patterns / read_patterns_from_file / pattern_insert / prepare_aho_automata
// (/root/reference/reads.cpp:253-267, 270-324, 330-410).  The reference builds a pointer trie,
// fail links and then rewrites child[] in place; here the DFA rows are produced directly in BFS
// order so that state id == the reference's BFS `id`: ids grow with the depth, and the states of
// one depth are numbered in the order of their strings -- what the tokenizer's tables (WalkTables)
// are derived from.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace scalce {

constexpr uint32_t kNoOut = 0xFFFFFFFFu;
constexpr int kLevelShift = 25;  // outinfo = level << 25 | bucket rank
constexpr uint32_t kBucketMask = (1u << kLevelShift) - 1;

struct Automaton {
  std::vector<std::string> patterns;    // file order: the index stored in .scalcer
  std::vector<uint32_t> next;           // 4 transitions per state
  std::vector<uint32_t> outinfo;        // longest core that is a suffix of the state, or kNoOut
  std::vector<int32_t> bucket_pattern;  // bucket rank -> pattern index; last entry = root (0x3FFFFFFF)
  std::vector<int32_t> bucket_level;    // bucket rank -> core length; root 0
  std::vector<int32_t> pattern_bucket;  // pattern index -> bucket rank, -1 if shadowed by a later duplicate
  int n_states = 0;
  int n_buckets = 0;  // root excluded
  int min_level = 0, max_level = 0;
  std::string error;

  bool load_bin(const void *blob, size_t n);
  bool load_text(const char *text, size_t n);

 private:
  bool build();
};

// What the tokenizer walks read besides outinfo and the bucket tables: derived from the DFA on the host, uploaded as it is.
// The table alone selects the walk (SCALCE_WALK_* of scalce_hip.h):
//   KMER / KMER_T7  the k-mer block below shortcuts every transition out of a state of depth <= 7 (tokenize_kmer_pipe_k,
//                   tie_candidates_pipe_k); T7: some state of depth <= 7 has an output (a core of fewer than 8 bases), and
//                   the 7-mer entries carry a flag for it
//   ANCHOR          more than 400 000 states and no core under 6 bases: thousands of 8-mers fit the block, a million
//                   cores of 12-32 bases walk deeper than it reaches, and are searched from the occurrences' starts
//                   instead (tokenize_anchor_k), K = min(shortest core, 12)
// The k-mer block, 52 KB: t7[16384] u16 (state the 7-mer leads to from the root | has-output << 15) | bits8[2048] u32 (the
// 8-mer is a trie node) | out8[2048] u32 (... with an output) | rank8[2048] u16 (nodes in front of the word).
constexpr uint32_t KMER_T7_WORDS = 16384 / 2, KMER_BITS_WORDS = 2048, KMER_WORDS = KMER_T7_WORDS + 2 * KMER_BITS_WORDS + 2048 / 2;
constexpr uint32_t kAnchorMinStates = 400000;  // tables with MORE states than this take the anchor walk

struct WalkTables {
  int walk = 0;                 // SCALCE_WALK_KMER, _KMER_T7 or _ANCHOR
  std::vector<uint32_t> next;   // Automaton::next with bit 31 set where the target state has an output (itself or through a
                                // suffix): the walks look the output up only where there is one (~1 % of a read's positions)
  std::vector<uint32_t> kmer;   // KMER_WORDS
  uint32_t id8_first = 0;       // first state of depth >= 8 (= n_states when there is none): depth >= 8 <=> id >= this
  // ANCHOR only
  uint32_t K = 0, idK = 0;              // anchor length; first state of depth K (they are idK .. idK + nodes - 1, in K-mer order)
  std::vector<uint64_t> anchor_bits;    // 4^K bits: the K-mer is a trie node
  std::vector<uint32_t> anchor_rank;    // per 64-bit word: nodes in front of it
  std::vector<uint32_t> child_bits;     // bit 4 s + c: transition c of state s is a trie edge
  std::vector<uint32_t> anchor_single;  // 4 words per depth-K node: {length | bucket << 6, suffix lo, suffix hi, 0} of the ONE
                                        // core below it, or 0 = walk down the trie
};
// false (and `error`) when the DFA breaks an invariant of the BFS numbering: not reached from a table Automaton::load_* built
bool build_walk_tables(const Automaton &A, WalkTables &T, std::string &error);

inline int base2(unsigned char c) {  // getval / _tbl, const.cpp:47-49 (bytes outside 'A'..'z': 0)
  switch (c) {
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 0;
  }
}

}  // namespace scalce
