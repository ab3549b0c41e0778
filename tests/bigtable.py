"""A core table of realistic size for tests and tools: up to 5 M cores of up to 32 bases are what the reference's loader
admits (/root/reference/reads.cpp:336,353-358); the table every other test uses has 15 600 cores of 8-12 bases."""
import itertools
import struct

import numpy as np

GROUPS_1M = ((12, 200_000), (14, 150_000), (16, 150_000), (18, 100_000), (20, 100_000), (24, 100_000), (28, 100_000), (32, 100_000))


def build(groups=GROUPS_1M, seed=99):
    """-> (patterns.bin blob, list of (length, values uint64 sorted ascending))"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    vals = []
    for ln, cnt in groups:
        hi = (1 << (2 * ln)) - 1
        v = np.unique(rng.integers(0, hi, size=int(cnt * 1.02) + 16, dtype=np.uint64, endpoint=True))
        v = np.sort(rng.permutation(v)[:cnt])
        assert len(v) == cnt
        nb = (ln + 3) // 4
        out += struct.pack("<hi", ln, cnt)
        out += v.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :nb].tobytes()
        vals.append((ln, v))
    return bytes(out), vals


def bases_of(ln, v):
    """(len(v), ln) uint8 ASCII: base j = (x >> 2 (ln - 1 - j)) & 3 (reads.cpp:346-364)"""
    shifts = (2 * (ln - 1 - np.arange(ln))).astype(np.uint64)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[((v[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]


def reads_with_cores(n, L, vals, seed=5, planted=0.7, n_frac=0.002):
    """n x L random reads; `planted` of them carry a core of the table at a random place (others may by chance)"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))]
    which = rng.random(n) < planted
    grp = rng.integers(0, len(vals), size=n)
    for g, (ln, v) in enumerate(vals):
        rows = np.flatnonzero(which & (grp == g))
        if not len(rows):
            continue
        pats = bases_of(ln, v[rng.integers(0, len(v), size=len(rows))])
        at = rng.integers(0, L - ln + 1, size=len(rows))
        idx = at[:, None] + np.arange(ln)[None, :]
        bases[rows[:, None], idx] = pats
    if n_frac:
        bases[rng.random((n, L)) < n_frac] = ord("N")
    return bases


# ---- core tables shaped for the tokenizer's walks (tests/test_gpu_tokenizer_tables.py, tests/test_ref_tables.py) --------
# The walk is chosen by the table alone (scalce_patterns_walk): k-mer tables when the automaton has at most 400 000 states
# or a core shorter than 6 bases, with T7 when a core is shorter than 8 bases; anchors of K = min(shortest core, 12) bases
# otherwise.  Every shape below names the walk it is built to select; the tests ask the library, never this rule.
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_DIGIT = str.maketrans("ACGT", "0123")
ANCHOR_THRESHOLD = 400_000


class Table:
    """A core table in file order.  text=False: written as patterns.bin (groups of one length, in the order given);
    text=True: a whitespace-separated list (any length, duplicates allowed: a later identical core wins)."""

    def __init__(self, name, cores, text, walk, note=""):
        self.name, self.cores, self.text, self.walk, self.note = name, list(cores), text, walk, note

    @property
    def blob(self):
        return text_of(self.cores) if self.text else bin_of(self.cores)

    @property
    def min_len(self):
        return min(len(c) for c in self.cores)


def text_of(cores):
    return ("\n".join(cores) + "\n").encode()


def bin_of(cores):
    """patterns.bin of cores of 1..32 bases; consecutive cores of one length form a group, file order kept"""
    out = bytearray()
    i = 0
    while i < len(cores):
        ln = len(cores[i])
        j = i
        while j < len(cores) and len(cores[j]) == ln:
            j += 1
        assert 1 <= ln <= 32
        nb = (ln + 3) // 4
        out += struct.pack("<hi", ln, j - i)
        for c in cores[i:j]:
            out += int(c.translate(_DIGIT), 4).to_bytes(8, "little")[:nb]
        i = j
    return bytes(out)


def random_cores(rng, ln, cnt):
    """cnt distinct random cores of ln bases (every one of them when cnt >= 4^ln)"""
    if ln <= 30 and cnt >= 4 ** ln:
        return ["".join(x) for x in itertools.product("ACGT", repeat=ln)]
    if ln <= 12:
        return [r.tobytes().decode() for r in bases_of(ln, rng.choice(4 ** ln, size=cnt, replace=False).astype(np.uint64))]
    if ln <= 32:
        hi = (1 << (2 * ln)) - 1
        v = np.unique(rng.integers(0, hi, size=int(cnt * 1.05) + 16, dtype=np.uint64, endpoint=True))
        v = rng.permutation(v)[:cnt]
        assert len(v) == cnt
        return [r.tobytes().decode() for r in bases_of(ln, v)]
    return [ACGT[rng.integers(0, 4, size=ln)].tobytes().decode() for _ in range(cnt)]


def n_states(cores):
    """automaton states (root included) = distinct prefixes of the cores"""
    seen = set()
    for c in cores:
        for d in range(1, len(c) + 1):
            seen.add(c[:d])
    return len(seen) + 1


def _threshold_pair(seed):
    """Cores of 16 bases whose automaton has exactly ANCHOR_THRESHOLD states, and the same cores plus one that adds a
    single state (a sibling of a leaf)."""
    rng = np.random.default_rng(seed)
    pool = random_cores(rng, 16, 60_000)
    seen, cores = set(), []
    for c in pool:
        new = [c[:d] for d in range(1, 17) if c[:d] not in seen]
        if 1 + len(seen) + len(new) > ANCHOR_THRESHOLD:
            break
        seen.update(new)
        cores.append(c)

    def branch(k):  # a core that leaves an existing one at depth 16 - k: exactly k new states
        for c in cores:
            p = 16 - k
            for x in "ACGT":
                if c[:p] + x not in seen:
                    tail = ACGT[rng.integers(0, 4, size=k - 1)].tobytes().decode()
                    return c[:p] + x + tail
        raise AssertionError("no free branch")
    gap = ANCHOR_THRESHOLD - (1 + len(seen))
    if gap:
        c = branch(gap)
        seen.update(c[:d] for d in range(1, 17))
        cores.append(c)
    assert 1 + len(seen) == ANCHOR_THRESHOLD
    return cores, cores + [branch(1)]


def _nested(rng, base, k):
    """cores around some of `base`: prefixes (one ends at depth k itself), suffixes that end on the same base as the
    longer core, and branches right below depth k -- nodes with more than one core below them, walked down the trie"""
    out = []
    long_ones = [c for c in base if len(c) >= k + 4]
    for c in long_ones[: len(long_ones) // 4]:
        x = "ACGT"[(("ACGT".index(c[k]) + 1 + int(rng.integers(0, 3))) % 4)]
        tail = ACGT[rng.integers(0, 4, size=int(rng.integers(0, 10)))].tobytes().decode()
        out += [c[:k], c[:k + 1], c[:-1], c[1:], c[-k:], c[:k] + x + tail]
    return out


def _long_text(rng, n_long, n_mid, n_dup):
    cores = []
    for ln in (44, 45):   # the longest suffix one record can hold at K = 12 (32 bases), and one base more
        cores += random_cores(rng, ln, n_long // 20)
    for ln in rng.integers(33, 128, size=n_long):
        cores.append(ACGT[rng.integers(0, 4, size=int(ln))].tobytes().decode())
    cores.append("T" * 127)
    for ln in (12, 16, 20, 32):
        cores += random_cores(rng, ln, n_mid)
    dup = [cores[int(i)] for i in rng.integers(0, len(cores), size=n_dup)]
    return cores + dup


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)   # (seeded by the name: a shape is the same table in every run)
    if name == "short_t7":       # cores of 1-7 bases (the single core A among them) beside 8-14
        cores = ["A"]
        for ln, cnt in ((2, 3), (3, 8), (4, 30), (5, 120), (6, 400), (7, 1500)):
            cores += random_cores(rng, ln, cnt)
        for ln in range(8, 15):
            cores += random_cores(rng, ln, 8000)
        return Table(name, cores, False, ("kmer_t7", 0))
    if name == "all8":           # every 8-mer: the depth-8 bitmap full, its rank at the top of its u16 range
        return Table(name, random_cores(rng, 8, 1 << 16), False, ("kmer", 0))
    if name == "all8_plus":      # every 8-mer and longer cores on top of them
        cores = random_cores(rng, 8, 1 << 16)
        for ln in range(9, 15):
            cores += random_cores(rng, ln, 4000)
        return Table(name, cores, False, ("kmer", 0))
    if name == "big_kmer":       # more than a million states, and one core of 5 bases: too short for anchors
        cores = random_cores(rng, 5, 1)
        for ln in range(28, 33):
            cores += random_cores(rng, ln, 10_000)
        return Table(name, cores, False, ("kmer_t7", 0), "states>=1M")
    if name in ("edge_under", "edge_over"):
        under, over = _threshold_pair(4711)
        return Table(name, under if name == "edge_under" else over, False,
                     ("kmer", 0) if name == "edge_under" else ("anchor", 12),
                     "states==%d" % (ANCHOR_THRESHOLD + (name == "edge_over")))
    if name == "anchor_k6":      # K = 6: a few thousand cores at depth K, nearly every depth-K node branches
        cores = random_cores(rng, 6, 300) + random_cores(rng, 7, 1500)
        for ln in (10, 14, 21, 22, 23, 26):
            cores += random_cores(rng, ln, 11_000)
        return Table(name, cores, False, ("anchor", 6))
    if name == "anchor_k8":
        cores = random_cores(rng, 8, 3000)
        for ln in (9, 12, 23, 24, 25, 28, 32):
            cores += random_cores(rng, ln, 9000)
        return Table(name, cores, False, ("anchor", 8))
    if name == "anchor_k11":     # a text list; its cores reach past 32 bases
        cores = []
        for ln in (11, 12, 19, 26, 27, 28, 31, 40):
            cores += random_cores(rng, ln, 8000)
        return Table(name, cores, True, ("anchor", 11))
    if name == "single":         # K = 12, suffixes of len - K = 0, 1, 15, 16, 17, 20 bases behind the anchor: one record each
        cores = []
        for ln in (12, 13, 27, 28, 29, 32):
            cores += random_cores(rng, ln, 12_000)
        return Table(name, cores, False, ("anchor", 12))
    if name == "anchor_min14":   # K = 12 with no core at depth K: the shortest core is longer than the anchor
        cores = []
        for ln in (14, 15, 18, 24):
            cores += random_cores(rng, ln, 15_000)
        return Table(name, cores, False, ("anchor", 12))
    if name == "nested":         # K = 10: cores that are prefixes / suffixes of longer ones, branches below depth K
        base = []
        for ln in range(10, 31, 2):
            base += random_cores(rng, ln, 4500)
        return Table(name, base + _nested(rng, base, 10), True, ("anchor", 10))
    if name == "long_text_anchor":   # text list of cores up to 127 bases (and duplicates): anchors
        return Table(name, _long_text(rng, 5000, 3000, 400), True, ("anchor", 12))
    if name == "long_text_kmer":     # the same kind of list, small enough for the k-mer walk
        return Table(name, _long_text(rng, 1500, 1500, 200), True, ("kmer", 0))
    raise KeyError(name)


SHAPES = ("short_t7", "all8", "all8_plus", "big_kmer", "edge_under", "edge_over", "anchor_k6", "anchor_k8", "anchor_k11",
          "single", "anchor_min14", "nested", "long_text_anchor", "long_text_kmer")
_TABLES = {}


def shape(name):
    """the table of a shape, built once per process"""
    if name not in _TABLES:
        _TABLES[name] = _build(name)
    return _TABLES[name]


def read_lengths(k):
    """lengths at which the walks' corners sit: one base short of an anchor, an anchor, a 32-bit word of bases and one
    base either side, a 128-position probe segment and one base either side, several segments"""
    return sorted({k - 1, k, 16, 17, 31, 32, 100, 128, 129, 250, 300})


def corner_reads(cores, L, n, seed, letters=True):
    """n x L reads (ASCII) carrying cores of the table where the kernels' corners are: at base 0, ending on the last base
    (the last rows of the batch as well), starting at every offset in a 16-base word, straddling the 128-position
    segments; and ties -- two distinct cores of one length, the same core twice.  Then N, lower-case and IUPAC
    letters."""
    rng = np.random.default_rng(seed)
    bases = ACGT[rng.integers(0, 4, size=(n, L))]
    by_len = {}
    for c in cores:
        if len(c) <= L:
            by_len.setdefault(len(c), []).append(c)
    lens = sorted(by_len)
    if lens:
        tail = max(16, n // 16)

        def put(r, c, at):
            bases[r, at:at + len(c)] = np.frombuffer(c.encode(), dtype=np.uint8)

        def pick(ln=None):
            ln = lens[int(rng.integers(0, len(lens)))] if ln is None else ln
            grp = by_len[ln]
            return grp[int(rng.integers(0, len(grp)))]
        for r in range(n):
            mode = 1 if r >= n - tail else r % 7
            c = pick()
            ln = len(c)
            if mode == 0:
                put(r, c, 0)
            elif mode == 1:
                put(r, c, L - ln)
            elif mode == 2:        # every start offset within a word of 16 bases (2 bits each), sh = 0 included
                starts = np.arange((r // 7) % 16, L - ln + 1, 16)
                if len(starts):
                    put(r, c, int(starts[rng.integers(0, len(starts))]))
            elif mode == 3:        # across a boundary of the anchor walk's 128-position segments
                bounds = [b for b in range(128, L, 128) if b - ln + 1 >= 0 and b - 1 + ln <= L]
                if bounds and ln > 1:
                    b = bounds[int(rng.integers(0, len(bounds)))]
                    put(r, c, int(rng.integers(b - ln + 1, min(b, L - ln + 1))))
                else:
                    put(r, c, int(rng.integers(0, L - ln + 1)))
            elif mode in (4, 5) and 2 * ln <= L:   # two distinct cores of one length / the same core twice
                d = pick(ln) if mode == 4 else c
                a = int(rng.integers(0, L - 2 * ln + 1))
                b = int(rng.integers(a + ln, L - ln + 1))
                if rng.random() < 0.5:
                    c, d = d, c
                put(r, c, a)
                put(r, d, b)
            else:
                put(r, c, int(rng.integers(0, L - ln + 1)))
    if letters:
        low = rng.random((n, L)) < 0.05
        bases = np.where(low, bases | 0x20, bases)
        amb = np.frombuffer(b"RYKMSWBDHVUXnryksw", dtype=np.uint8)
        hit = rng.random((n, L)) < 0.004
        bases = np.where(hit, amb[rng.integers(0, len(amb), size=(n, L))], bases)
        bases[rng.random((n, L)) < 0.003] = ord("N")
    return np.ascontiguousarray(bases, dtype=np.uint8)


def tie_reads(cores, L, n, seed, ncores=40):
    """n reads of L bases, each holding two of `ncores` cores of one length (the table's longest that fit twice): every
    read is a tie that the counts of the reads in front of it decide, and the lower-case / N letters of corner_reads"""
    rng = np.random.default_rng(seed)
    ln = max(len(c) for c in cores if 2 * len(c) <= L)
    grp = [c for c in cores if len(c) == ln]
    grp = [grp[int(i)] for i in rng.permutation(len(grp))[:ncores]]
    bases = ACGT[rng.integers(0, 4, size=(n, L))]
    arr = np.stack([np.frombuffer(c.encode(), dtype=np.uint8) for c in grp])
    i, j = rng.integers(0, len(grp), size=n), rng.integers(0, len(grp), size=n)
    a = rng.integers(0, L - 2 * ln + 1, size=n)
    b = a + ln + (rng.random(n) * (L - ln - (a + ln) + 1)).astype(np.int64)
    rows = np.arange(n)[:, None]
    bases[rows, a[:, None] + np.arange(ln)] = arr[i]
    bases[rows, b[:, None] + np.arange(ln)] = arr[j]
    bases[rng.random((n, L)) < 0.0005] = ord("N")
    return np.ascontiguousarray(bases, dtype=np.uint8)
