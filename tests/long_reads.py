"""Inputs at read lengths of 301 to 2498 bases, for tests/test_long_reads_cpu.py and tests/test_gpu_long_reads.py.

numpy and the oracle only, no GPU.  Every generator draws from one seed per case (the case's name and its arguments) and
returns (bases, quals) as n x L uint8 ASCII arrays.  What each case claims about itself -- where the cores end, which reads
tie, which runs the order stage meets -- is asserted with the oracle alone in test_long_reads_cpu.py, so that a GPU
comparison on these inputs cannot pass emptily."""
import functools
import os
import zlib

import numpy as np

import bigtable as B
import oraclelib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBIN = os.path.join(ROOT, "tests", "golden", "patterns.bin")
# both sides of the 128-position probe segments and of the 16-base words, the 2048 bit of a 12-bit position, the limit
LONG = [301, 511, 512, 513, 1000, 2047, 2048, 2049, 2432, 2433, 2497, 2498]
MAX_LENGTH = 2498            # batch_create refuses more: the reference reads lines into 2500 bytes
GENOME_BASES = 50_000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FILLERS = ("A", "C", "G", "T", "AC", "AG", "ACG")
END_TARGETS = (12, 255, 256, 257, 511, 512, 2047, 2048)   # and L - 1, L
HOMO_CORES = ("AAAAAAAA", "CCCCCCCC")


def seed_of(case, *args):
    return zlib.crc32(("%s:%s" % (case, ",".join(map(str, args)))).encode())


def random_quals(rng, shape):
    """quality characters from a span of 40, none at the offset"""
    return rng.integers(35, 75, size=shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shipped_table():
    """(blob, oracle trie, the 12-base cores as (file-order index, bytes)) of tests/golden/patterns.bin"""
    blob = open(PBIN, "rb").read()
    trie = O.Trie(blob=blob)
    lens = trie.pattern_lens()
    cores12 = [(int(p), trie.pattern(int(p))) for p in np.flatnonzero(lens == 12)]
    assert all(len(c) == 12 for _, c in cores12)
    return blob, trie, cores12


def row(text, L):
    return np.frombuffer((text * (L // len(text) + 1))[:L].encode(), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def filler_for(L):
    """the first of FILLERS that the oracle tokenises to "no core" at this length"""
    _, trie, _ = shipped_table()
    for f in FILLERS:
        pat, end = trie.tokenize(row(f, L)[None, :])
        if pat[0] < 0 and end[0] == 0:
            return f
    raise AssertionError("every filler holds a core of the table")


def place_core(rng, L, end, taken, filler=None):
    """a read of filler with one 12-base core of the table ending at `end`, which the oracle (counts at zero) gives exactly that
    core and end -- a junction with the filler may spell another core, then the next candidate is tried.
    -> (row, file-order index of the core)"""
    _, trie, cores12 = shipped_table()
    base = row(filler or filler_for(L), L)
    for k in rng.permutation(len(cores12)):
        p, core = cores12[int(k)]
        if p in taken:
            continue
        r = base.copy()
        r[end - 12:end] = np.frombuffer(core, dtype=np.uint8)
        pat, e = trie.tokenize(r[None, :])
        if pat[0] == p and e[0] == end:
            taken.add(p)
            return r, p
    raise AssertionError("no core of the table can be placed to end at %d" % end)


# ---- genome ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_genome():
    return ACGT[np.random.default_rng(seed_of("genome")).integers(0, 4, size=GENOME_BASES)]


def genome(n, L, seed=None, n_frac=0.003, dup_frac=0.1):
    """n reads cut from one 50 kb random genome -- cores repeat and reads overlap --, 0.3 % of the bases N, about a tenth of the
    reads whole-read duplicates of another one"""
    rng = np.random.default_rng(seed_of("genome", n, L) if seed is None else seed)
    g = shared_genome()
    start = rng.integers(0, GENOME_BASES - L + 1, size=n)
    bases = g[start[:, None] + np.arange(L)[None, :]]
    if n_frac:
        bases[rng.random((n, L)) < n_frac] = ord("N")
    k = int(n * dup_frac)
    if k and n > 1:                      # (behind the N: a duplicate is the whole read, its N included)
        bases[rng.integers(0, n, size=k)] = bases[rng.integers(0, n, size=k)]
    return np.ascontiguousarray(bases), random_quals(rng, (n, L))


# ---- ends -----------------------------------------------------------------------------------------------------------------
def end_targets(L):
    return sorted({e for e in END_TARGETS + (L - 1, L) if 12 <= e <= L})


def ends(L):
    """one read per target: filler with exactly one 12-base core, placed so that `end` is the target; then coreless reads (all
    filler, one per filler the oracle finds no core in) for the root bucket.  -> (bases, quals, targets, rows without a core)"""
    rng = np.random.default_rng(seed_of("ends", L))
    targets = end_targets(L)
    taken = set()
    rows = [place_core(rng, L, e, taken)[0] for e in targets]
    _, trie, _ = shipped_table()
    coreless = [row(f, L) for f in FILLERS[:4] if trie.tokenize(row(f, L)[None, :])[0][0] < 0] + [row(filler_for(L), L)]
    bases = np.stack(rows + coreless)
    order = rng.permutation(len(bases))
    return bases[order], random_quals(rng, bases.shape), targets, len(coreless)


# ---- many candidates ------------------------------------------------------------------------------------------------------
def many_candidates(L, n=16):
    """n reads, each the concatenation of L // 12 distinct 12-base cores of the table in an order of its own (filler behind
    them), drawn from a pool a quarter larger than one read holds, so that cores recur between reads: every read is a tie of
    about L / 12 candidates at the deepest level, decided by the counts of the reads in front of it"""
    rng = np.random.default_rng(seed_of("many_candidates", L))
    _, _, cores12 = shipped_table()
    k = L // 12
    pool = [cores12[int(i)][1] for i in rng.permutation(len(cores12))[:k + k // 4]]
    bases = np.empty((n, L), dtype=np.uint8)
    for r in range(n):
        pick = rng.permutation(len(pool))[:k]
        bases[r] = row(filler_for(L), L)
        bases[r, :12 * k] = np.frombuffer(b"".join(pool[int(i)] for i in pick), dtype=np.uint8)
    return bases, random_quals(rng, bases.shape)


# ---- a table with homopolymer cores ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def homopolymer_table(walk="kmer"):
    """A text core list with the two 8-base cores AAAAAAAA and CCCCCCCC and enough ordinary cores to select `walk` ("kmer":
    few states; "anchor": more than bigtable.ANCHOR_THRESHOLD states and no core shorter than 8, so anchors of 8 bases).  No
    ordinary core is spelt by a run of A next to a run of C.  -> the text"""
    rng = np.random.default_rng(seed_of("homopolymer_table", walk))
    groups = ((12, 4000),) if walk == "kmer" else ((12, 9000), (24, 9000), (28, 9000), (32, 9000))
    ac, ca = "A" * 40 + "C" * 40, "C" * 40 + "A" * 40
    cores = list(HOMO_CORES)
    for ln, cnt in groups:
        cores += [c for c in B.random_cores(rng, ln, cnt) if c not in ac and c not in ca]
    if walk == "anchor":
        assert B.n_states(cores) > B.ANCHOR_THRESHOLD
    return B.text_of(cores)


HOMO_KINDS = ("A", "AC", "CA", "C", "C", "C", "AC", "CA", "A", "CA", "AC", "C")


def homopolymer_reads(L):
    """reads for homopolymer_table: "A" / "C" all one letter -- L - 7 hits of one core, no tie --, "AC" half A then half C --
    a tie of the two cores with L - 14 candidate positions --, "CA" the halves swapped.  -> (bases, quals, kinds)"""
    rng = np.random.default_rng(seed_of("homopolymer_reads", L))
    h = L // 2
    rows = []
    for kind in HOMO_KINDS:
        r = row(kind[0], L)
        if len(kind) == 2:
            r[h:] = ord(kind[1])
        rows.append(r)
    bases = np.stack(rows)
    return bases, random_quals(rng, bases.shape), HOMO_KINDS


def homopolymer_expectation(kinds, L):
    """(core, end) per read by the reference's rule (aho_search, reads.cpp:413-429): the first hit of the deepest level stays
    unless a later core of that level has been chosen strictly more often by the reads in front"""
    count = {"A": 0, "C": 0}
    out = []
    for kind in kinds:
        pick, end = kind[0], 8
        if len(kind) == 2 and count[kind[1]] > count[kind[0]]:
            pick, end = kind[1], L // 2 + 8
        count[pick] += 1
        out.append((HOMO_CORES[0] if pick == "A" else HOMO_CORES[1], end))
    return out


# ---- runs that tie on the sort prefix -------------------------------------------------------------------------------------
RUN_SIZES = (5, 32, 40)
KEY_DIGIT_BASES = 4


def prefix_runs(L):
    """Three groups of reads -- 5, 32 and 40 members -- that share bucket, `end` (12: the core opens the read) and the first 16
    key bases.  Members differ only in the last base of the read and, where the read is long enough, in one base past key digit
    600; each group holds exact duplicates.  Input order is shuffled.
    -> (bases, quals, group of every read, the positions that differ)"""
    rng = np.random.default_rng(seed_of("prefix_runs", L))
    taken = set()
    far = 12 + KEY_DIGIT_BASES * 601 + 1     # a base inside key digit 601
    where = [L - 1] if far >= L - 1 else [far, L - 1]
    rows, group = [], []
    for g, size in enumerate(RUN_SIZES):
        base, _ = place_core(rng, L, 12, taken)
        members = [ACGT[rng.integers(0, 4, size=len(where))] for _ in range(size - 1)]
        members.append(members[0])           # two exact duplicates at the least
        for m in members:
            r = base.copy()
            r[where] = m
            rows.append(r)
            group.append(g)
    order = rng.permutation(len(rows))
    bases = np.stack(rows)[order]
    return bases, random_quals(rng, bases.shape), np.array(group)[order], where


# ---- variable length ------------------------------------------------------------------------------------------------------
def varlen_lengths(L):
    """0, 1, 15, 16, 17, 255, 256, 257, 2047, 2048, L - 1, L (those up to L) and random lengths, permuted; as many of them
    that the records of varlen_util.texts (names "v.<i>") begin on every byte phase 0 .. 15"""
    rng = np.random.default_rng(seed_of("varlen_lengths", L))
    fixed = sorted({k for k in (0, 1, 15, 16, 17, 255, 256, 257, 2047, 2048, L - 1, L) if 0 <= k <= L})
    n = len(fixed) + 12
    while True:
        lens = rng.permutation(np.concatenate([fixed, rng.integers(0, L + 1, size=n - len(fixed))])).astype(np.int64)
        starts = np.cumsum([0] + [2 * int(k) + len("v.%d" % i) + 6 for i, k in enumerate(lens)])[:-1]
        if len(set(int(s) % 16 for s in starts)) == 16:
            return lens
        n += 4


# ---- letters and qualities the archive does not keep ----------------------------------------------------------------------
def exception_patterns(L, n=70):
    """reads without N and without a quality at the offset, then: read 0 lower-case at positions 0, 2047, 2048 and L - 1, read 1
    entirely lower-case, read 2 all N with a quality above the offset throughout, and one exception in a hundred positions of
    the others (lower-case, N, IUPAC letters, the offset quality).  -> (bases, quals, the positions of read 0)"""
    rng = np.random.default_rng(seed_of("exception_patterns", L))
    bases, quals = genome(n, L, seed=seed_of("exception_patterns/genome", L), n_frac=0)
    bases, quals = bases.copy(), quals.copy()
    hit = rng.random(bases.shape) < 0.01
    hit[:3] = False
    kind = rng.integers(0, 4, bases.shape)
    odd = np.frombuffer(b"RYKMSWBDHVUXryksw", dtype=np.uint8)
    bases[hit & (kind == 0)] |= 0x20
    bases[hit & (kind == 1)] = ord("N")
    bases[hit & (kind == 2)] = odd[rng.integers(0, len(odd), int((hit & (kind == 2)).sum()))]
    quals[hit & (kind == 3)] = ord("!")
    at = [p for p in (0, 2047, 2048, L - 1) if p < L]
    bases[0, at] |= 0x20
    bases[1] |= 0x20
    bases[2] = ord("N")
    return bases, quals, at


def fastq(bases, quals, prefix="s.", suffix="", lens=None, comments=False):
    """the FASTQ text of the arrays: names "<prefix><i><suffix>", a bare '+' line; lens: each read cut to its length"""
    out = []
    for i in range(len(bases)):
        k = bases.shape[1] if lens is None else int(lens[i])
        head = b"@" + prefix.encode() + b"%d" % i + suffix.encode() + (b" 1:N:0:ACGT len=%d" % k if comments and i % 3 else b"")
        out.append(head + b"\n" + bases[i, :k].tobytes() + b"\n+\n" + quals[i, :k].tobytes() + b"\n")
    return b"".join(out)
