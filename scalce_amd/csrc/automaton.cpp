#include "automaton.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/scalce_hip.h"

namespace scalce {

bool Automaton::load_bin(const void *blob, size_t n) {
  // [int16 len][int32 count] + count little-endian integers of ceil(len/4) bytes whose most
  // significant 2-bit digit is the first base (reads.cpp:342-364)
  const uint8_t *p = static_cast<const uint8_t *>(blob);
  size_t pos = 0;
  patterns.clear();
  while (pos < n) {
    if (pos + 6 > n) { error = "truncated group header in core table"; return false; }
    int16_t ln; int32_t cnt;
    std::memcpy(&ln, p + pos, 2);
    std::memcpy(&cnt, p + pos + 2, 4);
    pos += 6;
    if (ln <= 0 || ln > 32 || cnt < 0) { error = "core length outside 1..32 in core table"; return false; }
    const size_t nb = (size_t(ln) + 3) / 4;
    if (pos + nb * size_t(cnt) > n) { error = "truncated group in core table"; return false; }
    for (int32_t i = 0; i < cnt; i++, pos += nb) {
      uint64_t x = 0;
      std::memcpy(&x, p + pos, nb);
      std::string s(size_t(ln), 'A');
      for (int j = 0; j < ln; j++) s[j] = "ACGT"[(x >> (2 * (ln - 1 - j))) & 3];
      patterns.push_back(std::move(s));
    }
  }
  return build();
}

bool Automaton::load_text(const char *text, size_t n) {
  patterns.clear();
  size_t i = 0;
  auto ws = [](char c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r' || c == '\f' || c == '\v'; };
  while (i < n) {
    while (i < n && ws(text[i])) i++;
    size_t s = i;
    while (i < n && !ws(text[i])) i++;
    if (i > s) patterns.emplace_back(text + s, i - s);
  }
  return build();
}

bool Automaton::build() {
  struct Node { int32_t child[4]; int32_t output; int32_t level; };
  std::vector<Node> trie(1, Node{{-1, -1, -1, -1}, -1, 0});
  for (size_t p = 0; p < patterns.size(); p++) {
    int cur = 0;
    for (unsigned char ch : patterns[p]) {
      int c = base2(ch);
      if (trie[cur].child[c] < 0) {
        trie[cur].child[c] = int32_t(trie.size());
        trie.push_back(Node{{-1, -1, -1, -1}, -1, trie[cur].level + 1});
      }
      cur = trie[cur].child[c];
    }
    trie[cur].output = int32_t(p);  // a later identical core wins (reads.cpp:264)
  }
  n_states = int(trie.size());
  // BFS numbering, children visited A,C,G,T: rank == the reference's `id` (reads.cpp:275-297)
  std::vector<int32_t> order;
  order.reserve(trie.size());
  std::vector<int32_t> newid(trie.size(), -1);
  order.push_back(0);
  newid[0] = 0;
  for (size_t h = 0; h < order.size(); h++)
    for (int c = 0; c < 4; c++) {
      int32_t ch = trie[order[h]].child[c];
      if (ch >= 0) { newid[ch] = int32_t(order.size()); order.push_back(ch); }
    }
  // bucket rank = rank among core-ending states in id order = emission order of aho_output
  pattern_bucket.assign(patterns.size(), -1);
  bucket_pattern.clear();
  bucket_level.clear();
  std::vector<int32_t> state_bucket(trie.size(), -1);
  min_level = 1 << 30; max_level = 0;
  for (size_t s = 0; s < order.size(); s++) {
    const Node &nd = trie[order[s]];
    if (nd.output >= 0 && s != 0) {
      state_bucket[s] = int32_t(bucket_pattern.size());
      pattern_bucket[nd.output] = state_bucket[s];
      bucket_pattern.push_back(nd.output);
      bucket_level.push_back(nd.level);
      if (nd.level < min_level) min_level = nd.level;
      if (nd.level > max_level) max_level = nd.level;
    }
  }
  n_buckets = int(bucket_pattern.size());
  if (n_buckets == 0) min_level = 0;
  if (max_level > 127) { error = "core longer than 127 bases"; return false; }
  if (n_buckets >= int(kBucketMask)) { error = "too many cores"; return false; }
  bucket_pattern.push_back(0x3FFFFFFF);  // root bucket, dumped last (reads.cpp:491-495,161-164)
  bucket_level.push_back(0);
  // total transition function + longest-suffix core per state, rows filled in BFS order
  next.assign(size_t(n_states) * 4, 0);
  outinfo.assign(size_t(n_states), kNoOut);
  std::vector<int32_t> fail(trie.size(), 0), outst(trie.size(), -1);
  for (size_t s = 0; s < order.size(); s++) {
    const Node &nd = trie[order[s]];
    const int32_t f = fail[s];
    outst[s] = (s != 0 && nd.output >= 0) ? int32_t(s) : (s == 0 ? -1 : outst[f]);
    if (outst[s] >= 0) {
      const int32_t b = state_bucket[outst[s]];
      outinfo[s] = (uint32_t(bucket_level[b]) << kLevelShift) | uint32_t(b);
    }
    for (int c = 0; c < 4; c++) {
      const int32_t ch = nd.child[c];
      if (ch >= 0) {
        const int32_t t = newid[ch];
        next[s * 4 + c] = uint32_t(t);
        fail[t] = (s == 0) ? 0 : int32_t(next[size_t(f) * 4 + c]);
      } else {
        next[s * 4 + c] = (s == 0) ? 0u : next[size_t(f) * 4 + c];
      }
    }
  }
  return true;
}

bool build_walk_tables(const Automaton &A, WalkTables &T, std::string &error) {
  const uint32_t ns = uint32_t(A.n_states);
  auto broken = [&](const char *what) {
    error = std::string("core table: the automaton is not numbered in BFS order (") + what + ")";
    return false;
  };
  T = WalkTables();
  T.next = A.next;
  for (auto &t : T.next)
    if (A.outinfo[t] != kNoOut) t |= 0x80000000u;
  // Depth of every state = its distance from the root (a transition raises the depth by at most one and the trie path
  // does); the string of a state follows its first discovery.
  std::vector<int> depth(ns, -1);
  std::vector<uint32_t> code(ns, 0), order;
  order.reserve(ns);
  depth[0] = 0;
  order.push_back(0);
  for (size_t h = 0; h < order.size(); h++) {
    const uint32_t st = order[h];
    for (uint32_t ch = 0; ch < 4; ch++) {
      const uint32_t t = A.next[size_t(st) * 4 + ch];
      if (depth[t] < 0) { depth[t] = depth[st] + 1; code[t] = (code[st] << 2) | ch; order.push_back(t); }
    }
  }
  if (order.size() != ns) return broken("a state is not reachable");
  uint32_t id8 = ns, n8 = 0;
  for (uint32_t st = 0; st < ns; st++) {  // ids are BFS ranks: depth must not decrease with the id
    if (st && depth[st] < depth[st - 1]) return broken("depth decreases with the id");
    if (depth[st] >= 8 && id8 == ns) id8 = st;
    if (depth[st] == 8) n8++;
  }
  if (id8 > 32768) return broken("more than 32768 states of depth <= 7");  // t7 keeps a state in 15 bits
  T.id8_first = id8;
  T.kmer.assign(KMER_WORDS, 0);
  bool t7_out = false;  // a state of depth <= 7 with an output (a core of fewer than 8 bases in the table)
  {
    uint16_t *t7 = reinterpret_cast<uint16_t *>(T.kmer.data());
    uint32_t *bits8 = T.kmer.data() + KMER_T7_WORDS, *out8 = bits8 + KMER_BITS_WORDS;
    uint16_t *rank8 = reinterpret_cast<uint16_t *>(out8 + KMER_BITS_WORDS);
    for (uint32_t x = 0; x < 16384; x++) {
      uint32_t st = 0;
      for (int j = 0; j < 7; j++) st = A.next[size_t(st) * 4 + ((x >> (12 - 2 * j)) & 3)];
      if (st >= 32768 || st >= id8) return broken("seven bases lead below depth 7");
      t7[x] = uint16_t(st | (A.outinfo[st] != kNoOut ? 0x8000u : 0u));
      if (A.outinfo[st] != kNoOut) t7_out = true;
    }
    uint32_t prev_code = 0;
    for (uint32_t i = 0; i < n8; i++) {  // the depth-8 states: ids id8 .. id8 + n8 - 1 in the order of their 8-mers
      const uint32_t st = id8 + i;
      if (st >= ns || depth[st] != 8 || (i && code[st] <= prev_code)) return broken("states of depth 8 are not in 8-mer order");
      prev_code = code[st];
      bits8[code[st] >> 5] |= 1u << (code[st] & 31);
      if (A.outinfo[st] != kNoOut) out8[code[st] >> 5] |= 1u << (code[st] & 31);
    }
    uint32_t run = 0;
    for (uint32_t wi = 0; wi < KMER_BITS_WORDS; wi++) {
      if (run > 0xFFFF) return broken("rank of an 8-mer beyond 16 bits");
      rank8[wi] = uint16_t(run);
      run += uint32_t(__builtin_popcount(bits8[wi]));
    }
  }
  T.walk = t7_out ? SCALCE_WALK_KMER_T7 : SCALCE_WALK_KMER;
  // Anchor tables.  (The k-mer block only shortcuts transitions out of states of depth <= 7: with more than 400 000 states
  // most of the walk is deeper than that.)
  if (!(ns > kAnchorMinStates && A.min_level >= 6 && A.n_buckets > 0)) return true;
  const uint32_t K = uint32_t(std::min(A.min_level, 12));
  const size_t nbits = size_t(1) << (2 * K), nwords = (nbits + 63) / 64;
  T.anchor_bits.assign(nwords, 0);
  uint32_t idK = ns, nK = 0, prev = 0;
  for (uint32_t st = 0; st < ns; st++) {  // ids of depth K: one contiguous range (depth grows with the id) in K-mer order
    if (depth[st] != int(K)) continue;
    if (idK == ns) idK = st;
    else if (code[st] <= prev) return broken("states of the anchor depth are not in K-mer order");
    prev = code[st];
    nK++;
    T.anchor_bits[code[st] >> 6] |= 1ull << (code[st] & 63u);
  }
  if (idK == ns) return broken("no state of the anchor depth");
  T.anchor_rank.resize(nwords);
  uint32_t run = 0;
  for (size_t w = 0; w < nwords; w++) { T.anchor_rank[w] = run; run += uint32_t(__builtin_popcountll(T.anchor_bits[w])); }
  T.child_bits.assign((size_t(ns) * 4 + 31) / 32, 0);
  for (uint32_t st = 0; st < ns; st++)
    for (uint32_t ch = 0; ch < 4; ch++) {
      const uint32_t t = A.next[size_t(st) * 4 + ch];
      if (depth[t] == depth[st] + 1) T.child_bits[(size_t(st) * 4 + ch) >> 5] |= 1u << ((size_t(st) * 4 + ch) & 31);
    }
  // One probe for most anchors.  Below 97 % of the depth-K nodes of a million-core table hangs exactly ONE core, on a path
  // without branches: for those the walk down the trie (three dependent loads per base, up to 20 bases) is one 16-byte
  // record -- length, bucket, the bases behind the K-mer packed like the K-mer itself -- and one comparison with the read's
  // own bits.  Any other node (branches, a core that is a prefix of another) keeps record 0 and is walked.
  T.anchor_single.assign(size_t(nK) * 4, 0);
  for (uint32_t j = 0; j < nK; j++) {
    uint32_t st = idK + j, d = K, cores = 0, bucket = 0, len = 0;
    uint64_t suf = 0;
    bool simple = true;
    for (;;) {
      const uint32_t info = A.outinfo[st];
      if (info != kNoOut && (info >> kLevelShift) == d) { cores++; bucket = info & kBucketMask; len = d; }
      uint32_t nch = 0, chv = 0, nxt = 0;
      for (uint32_t ch = 0; ch < 4; ch++) {
        const uint32_t t = A.next[size_t(st) * 4 + ch];
        if (depth[t] == depth[st] + 1) { nch++; chv = ch; nxt = t; }
      }
      if (nch == 0) break;
      if (nch > 1 || cores) { simple = false; break; }   // a branch, or a core with more cores below it
      suf = (suf << 2) | chv;
      st = nxt;
      d++;
      if (d > 44) { simple = false; break; }
    }
    if (simple && cores == 1 && len == d && len - K <= 32 && len < 64 && bucket < (1u << 26)) {
      T.anchor_single[size_t(j) * 4] = len | (bucket << 6);
      T.anchor_single[size_t(j) * 4 + 1] = uint32_t(suf);
      T.anchor_single[size_t(j) * 4 + 2] = uint32_t(suf >> 32);
    }
  }
  T.K = K;
  T.idK = idK;
  T.walk = SCALCE_WALK_ANCHOR;
  return true;
}

}  // namespace scalce
