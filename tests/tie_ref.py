"""The tie-break restated in plain Python: which core a read goes to when it holds several cores of the longest length.

A read belongs to the longest core that occurs in it.  Where several distinct cores of that length occur, they are taken
in the order of their first appearance and a later one replaces the one held only when its bucket holds STRICTLY more reads
so far (aho_search with the cumulative bin_size: the reads of earlier shards, and every read in front of this one, whatever
decided it).  Python integers throughout, no oracle and no device inside: tests/test_tie_ref_cpu.py holds these functions
against the oracle, tests/test_gpu_tie_break.py holds the device against them.

Patterns are indices into the core list in file order, ROOT (-1) is "no core occurs"; counts and priors are dicts
pattern -> reads (missing = 0)."""
import random
import struct

ROOT = -1


class Index:
    """cores by length, longest first: {core: pattern}; of two identical cores the later one of the list keeps the name"""

    def __init__(self, cores):
        self.cores = list(cores)
        by_len = {}
        for p, c in enumerate(self.cores):
            by_len.setdefault(len(c), {})[c] = p
        self.by_len = sorted(by_len.items(), reverse=True)


def cores_of_bin(blob):
    """the cores of a patterns.bin in file order: groups of [int16 length][int32 count] and count numbers of ceil(length / 4)
    bytes, little-endian, first base in the most significant digit"""
    out, pos = [], 0
    while pos + 6 <= len(blob):
        ln, cnt = struct.unpack_from("<hi", blob, pos)
        pos += 6
        nb = (ln + 3) // 4
        for _ in range(cnt):
            x = int.from_bytes(blob[pos:pos + nb], "little")
            pos += nb
            out.append("".join("ACGT"[(x >> (2 * (ln - 1 - j))) & 3] for j in range(ln)))
    return out


def as_text(read):
    return read if isinstance(read, str) else bytes(read).decode("ascii")


def occurrences(cores, read):
    """every occurrence of a core of the longest length that occurs in the read, by position: [(pattern, last base)]"""
    idx = cores if isinstance(cores, Index) else Index(cores)
    read = as_text(read)
    for ln, table in idx.by_len:
        hits = []
        for i in range(len(read) - ln + 1):
            p = table.get(read[i:i + ln])
            if p is not None:
                hits.append((p, i + ln - 1))
        if hits:
            return hits
    return []


def candidates(cores, read):
    """the distinct cores of the longest length occurring in the read, in order of first appearance, each with the index of
    the last base of its first occurrence: [(pattern, last base)]; [] when no core occurs"""
    seen, out = set(), []
    for p, e in occurrences(cores, read):
        if p not in seen:
            seen.add(p)
            out.append((p, e))
    return out


def _walk(cand_lists, fixed, prior):
    """The sequential rule.  Per read: (ordinal of the candidate taken or None, the counts of all candidates at the moment of
    the decision); and the counts of the reads walked plus `fixed`."""
    prior = prior or {}
    own = dict(fixed or {})
    steps = []
    for cands in cand_lists:
        if not cands:
            own[ROOT] = own.get(ROOT, 0) + 1
            steps.append((None, ()))
            continue
        seen = tuple(prior.get(p, 0) + own.get(p, 0) for p, _ in cands)
        best = 0
        for j in range(1, len(cands)):
            if seen[j] > seen[best]:
                best = j
        own[cands[best][0]] = own.get(cands[best][0], 0) + 1
        steps.append((best, seen))
    return steps, own


def settle(cand_lists, fixed=None, prior=None):
    """cand_lists[r] = candidates of read r (none: no core; one: a fixed read; more: a tie read), in input order.
    fixed: reads of the same batch that are in their buckets already, in front of these (the pieces before this one);
    prior: reads of earlier batches.  A bucket's count is prior + fixed + every read in front, fixed reads included.
    -> ([(pattern, end)] per read -- end = last base + 1, (ROOT, 0) without a core --, counts of the batch's own reads:
    `fixed` and the reads walked, without the prior)"""
    steps, own = _walk(cand_lists, fixed, prior)
    toks = [(ROOT, 0) if j is None else (c[j][0], c[j][1] + 1) for c, (j, _) in zip(cand_lists, steps)]
    return toks, {p: n for p, n in own.items() if n}


def choices(cand_lists, fixed=None, prior=None):
    """ordinal of the candidate taken, per read (None without a core)"""
    return [j for j, _ in _walk(cand_lists, fixed, prior)[0]]


def equal_count_decisions(cand_lists, fixed=None, prior=None):
    """(tie reads decided while two or more of their candidates shared the largest count -- the strict comparison decides --,
    tie reads)"""
    steps, _ = _walk(cand_lists, fixed, prior)
    ties = [(j, seen) for j, seen in steps if len(seen) > 1]
    return sum(1 for _, seen in ties if seen.count(max(seen)) > 1), len(ties)


def tie_rows(cand_lists):
    return [r for r, c in enumerate(cand_lists) if len(c) > 1]


def jacobi_sweeps(cand_lists, fixed=None, prior=None):
    """Global sweeps from the start "every read takes its first candidate": in a sweep every read decides again from the
    counts the PREVIOUS sweep's choices give the reads in front of it.  -> sweeps up to and including the first one that
    moves nothing.  (Chooses inputs; the fixed point itself is settle().)"""
    prior = prior or {}
    choice = [0 if c else None for c in cand_lists]
    sweeps = 0
    while True:
        sweeps += 1
        own = dict(fixed or {})
        new = []
        for cands, old in zip(cand_lists, choice):
            if not cands:
                new.append(None)
                continue
            best, bestc = 0, None
            for j, (p, _) in enumerate(cands):
                c = prior.get(p, 0) + own.get(p, 0)
                if bestc is None or c > bestc:
                    best, bestc = j, c
            new.append(best)
            own[cands[old][0]] = own.get(cands[old][0], 0) + 1
        if new == choice:
            return sweeps
        choice = new


# ---- inputs: upper-case ACGT only, a fixed seed --------------------------------------------------------------------------
def random_cores(seed, length, count, avoid=()):
    """`count` distinct random cores of `length` bases, none of them in `avoid`"""
    rng = random.Random(seed)
    out, seen = [], set(avoid)
    while len(out) < count:
        c = "".join(rng.choice("ACGT") for _ in range(length))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def plant(rng, L, cores):
    """a read of L random bases with `cores` (strings, in this order) at random places that do not overlap"""
    need = sum(len(c) for c in cores)
    assert need <= L, (need, L)
    gaps = sorted(rng.randint(0, L - need) for _ in cores)
    read = [rng.choice("ACGT") for _ in range(L)]
    at = 0
    for g, c in zip(gaps, cores):
        read[g + at:g + at + len(c)] = c
        at += len(c)
    return "".join(read)


def reads_with_cores(pool, L, n, seed, kmin=0, kmax=12, twice=0.3, fixed_frac=0.15, ascending=False, tie_first=False,
                     tie_last=False):
    """n reads of L bases.  A read holds k distinct cores of `pool` (strings of one length), k uniform in kmin .. kmax as far
    as L has room, some of them a second time (more hits than distinct candidates); fixed_frac of the reads hold one core.
    ascending: the cores of a read stand in the order of the pool.  tie_first / tie_last: row 0 / the last row hold two
    cores at least.  What a read really holds -- chance occurrences included -- is for candidates() to say."""
    rng = random.Random(seed)
    ln = len(pool[0])
    assert all(len(c) == ln for c in pool)
    reads = []
    for r in range(n):
        k = 1 if rng.random() < fixed_frac else rng.randint(kmin, kmax)
        if (r == 0 and tie_first) or (r == n - 1 and tie_last):
            k = max(k, 2)
        k = min(k, L // ln, len(pool))
        which = rng.sample(range(len(pool)), k)
        if ascending:
            which.sort()
        put = [pool[i] for i in which]
        for c in list(put):
            if rng.random() < twice and (len(put) + 1) * ln <= L:
                put.insert(rng.randint(put.index(c) + 1, len(put)), c)   # behind its first occurrence: the order stands
        reads.append(plant(rng, L, put))
    return reads


def doubling_reads(a, b, L, n, seed):
    """a read holding `b` alone, then n reads holding `a` in front of `b`: in input order every one of them goes to b (b is
    one ahead and stays ahead); global sweeps from "first candidate" get 1, 2, 4, 8 .. reads further per sweep"""
    rng = random.Random(seed)
    return [plant(rng, L, [b])] + [plant(rng, L, [a, b]) for _ in range(n)]


def fastq(reads):
    """the reads as FASTQ text: names r<row>, qualities I"""
    return "".join(f"@r{i}\n{as_text(r)}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()


# ---- the tables and inputs of tests/test_gpu_tie_break.py (tests/test_tie_ref_cpu.py holds each against the oracle) ------
class Table:
    """name, cores in file order, text list or patterns.bin, the blob the loaders take, the walk it is meant to select, and
    `pool`: cores of one length (no longer core is likely in a read) that the inputs are planted from"""

    def __init__(self, name, cores, text, blob, walk, pool):
        self.name, self.cores, self.text, self.blob, self.walk, self.pool = name, cores, text, blob, walk, pool
        self.index = Index(cores)
        self.pattern = {c: p for p, c in enumerate(cores)}

    def candidates(self, reads):
        return [candidates(self.index, r) for r in reads]


_TABLES, _INPUTS = {}, {}
TABLE_NAMES = ("t7", "ten", "anchor_k8", "patterns", "all8")


def table(name):
    if name in _TABLES:
        return _TABLES[name]
    if name == "t7":        # cores of 4, 5 and 7 bases: the k-mer walk with the 7-mer table's output flags
        cores = random_cores(101, 4, 6) + random_cores(102, 5, 10) + random_cores(103, 7, 160)
        t = Table(name, cores, True, ("\n".join(cores) + "\n").encode(), ("kmer_t7", 0), cores[16:])
    elif name == "ten":     # 160 cores of 10 bases: the k-mer walk.  (Many cores for the reads there are: a bucket holds a
        cores = random_cores(104, 10, 160)   # dozen reads, and a tenth of the decisions meet equal counts)
        t = Table(name, cores, True, ("\n".join(cores) + "\n").encode(), ("kmer", 0), cores)
    elif name == "patterns":   # the table of every other test: 15 600 cores of 8, 10 and 12 bases
        import os
        blob = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patterns.bin"), "rb").read()
        cores = cores_of_bin(blob)
        twelve = [c for c in cores if len(c) == 12]
        t = Table(name, cores, False, blob, ("kmer", 0), random.Random(105).sample(twelve, 40))
    else:
        import bigtable
        b = bigtable.shape(name)
        ln = 12 if name == "anchor_k8" else 8
        pool = random.Random(106).sample([c for c in b.cores if len(c) == ln], 48 if ln == 12 else 30)
        t = Table(name, b.cores, b.text, b.blob, b.walk, pool)
    _TABLES[name] = t
    return t


def periodic_reads(units, L, n, seed):
    """reads that repeat a unit of 1 .. 8 bases: such a read holds exactly as many distinct 8-mers as its unit is long (a
    unit that is itself periodic: fewer), each of them many times"""
    rng = random.Random(seed)
    return [(u * (L // len(u) + 1))[:L] for u in (rng.choice(units) for _ in range(n))]


def rank_prior(t):
    """the pool's cores counted 0, 1, 2 .. in pool order: in a read whose cores stand in that order every later candidate
    starts at least one ahead of the ones in front of it, the last one ahead of all"""
    return {t.pattern[c]: i for i, c in enumerate(t.pool)}


def inputs(name):
    """-> (Table, reads): the inputs by name, built once"""
    if name in _INPUTS:
        return _INPUTS[name]
    if name in ("walk_t7", "walk_ten", "walk_anchor_k8"):   # 0 .. 12 cores per read, some twice, tie reads on both end rows
        t = table(name[5:])
        L = {"walk_t7": 100, "walk_ten": 100, "walk_anchor_k8": 160}[name]
        reads = reads_with_cores(t.pool, L, 2048, seed=len(name), tie_first=True, tie_last=True)
    elif name in ("priors", "priors_prefix"):   # as walk_ten with the cores of a read in the order of the pool (rank_prior):
        t = table("ten")                        # 4096 reads, "priors" the second half, "priors_prefix" the half in front of it
        reads = reads_with_cores(t.pool, 100, 4096, seed=7, ascending=True)
        reads = reads[2048:] if name == "priors" else reads[:2048]
    elif name == "two":           # every tie read holds exactly two cores (8 to choose from); fixed reads between them
        t = table("ten")
        t8 = Table("ten", t.cores, t.text, t.blob, t.walk, t.pool[:8])
        reads = reads_with_cores(t8.pool, 40, 340, seed=8, kmin=2, kmax=2, twice=0.0, fixed_frac=0.3)
        reads = [r for r in reads if 1 <= len(candidates(t.index, r)) <= 2]   # (a third core by chance: not in this input)
        ties = [r for r, c in enumerate(t.candidates(reads)) if len(c) > 1]
        reads = reads[:ties[200]]       # 200 tie reads exactly, the fixed reads behind the last of them included
    elif name == "mixed":         # the first rows of walk_ten: candidate counts of every class in one small batch
        t, reads = inputs("walk_ten")
        reads = reads[:320]
    elif name in ("tie_first_only", "tie_last_only", "no_tie"):   # fixed reads, and one tie read on row 0 / the last row / nowhere
        t = table("ten")
        reads = reads_with_cores(t.pool, 40, 320, seed=9, kmin=1, kmax=1, twice=0.3, fixed_frac=0.0)
        reads = [r for r in reads if len(candidates(t.index, r)) == 1][:300]   # (a second core by chance: not in this input)
        both = plant(random.Random(10), 40, [t.pool[3], t.pool[1]])
        if name == "tie_first_only":
            reads[0] = both
        elif name == "tie_last_only":
            reads[-1] = both
    elif name == "doubling":      # global sweeps need six rounds; in input order every read goes to the second core
        t = table("ten")
        reads = doubling_reads(t.pool[0], t.pool[1], 40, 16, seed=11)
    elif name == "seq_patterns":  # the table whose counters need the raised LDS limit
        t = table("patterns")
        reads = reads_with_cores(t.pool, 100, 1024, seed=12, kmax=8)
    elif name == "seq_all8":      # every 8-mer is a core: a read of 40 bases holds up to 33 of them; periodic reads hold 1 .. 8
        t = table("all8")
        units = [u for k in range(1, 9) for u in random_cores(13 + k, k, min(6, 4 ** k))]
        reads = reads_with_cores(t.pool, 40, 512, seed=13, kmax=5) + periodic_reads(units, 40, 512, seed=14)
        random.Random(15).shuffle(reads)
    elif name == "cell_cap":      # two cores of the golden table per read: more windows of one read than 64 Mi cells hold
        t = table("patterns")
        reads = reads_with_cores(t.pool, 48, 4400, seed=16, kmin=2, kmax=2, twice=0.0, fixed_frac=0.0)
    else:
        raise KeyError(name)
    _INPUTS[name] = (t, reads)
    return _INPUTS[name]


INPUT_NAMES = ("walk_t7", "walk_ten", "walk_anchor_k8", "priors", "priors_prefix", "two", "mixed", "tie_first_only", "tie_last_only", "no_tie",
               "doubling", "seq_patterns", "seq_all8", "cell_cap")
_CANDS = {}


def input_candidates(name):
    """-> (Table, reads, candidate lists), computed once per process"""
    if name not in _CANDS:
        t, reads = inputs(name)
        _CANDS[name] = (t, reads, t.candidates(reads))
    return _CANDS[name]


def priors_under_test():
    """The priors the input "priors" is settled under: name -> (prior, must the decisions differ from those without one).
    Patterns not named count 0.  prefix: the counts of the 2048 reads in front of the input ("priors_prefix")."""
    t, _, in_front = input_candidates("priors_prefix")
    every = list(range(len(t.cores))) + [ROOT]
    rng = random.Random(17)
    return {
        "none": (None, False),
        "zero": ({p: 0 for p in every}, False),
        "prefix": (settle(in_front)[1], True),
        "equal": ({p: 1000 for p in every}, False),
        "last_ahead": (rank_prior(t), True),
        "above_2_33": ({p: (1 << 33) + 5 + rng.randint(0, 1) for p in every}, True),
        "root_only": ({ROOT: 12345}, False),
        # the upper 32 bits decide, the lower 32 bits alone would decide the other way round (a sum kept in 32 bits)
        "high_bits": ({p: ((p % 5) << 32) + 1000 * (4 - p % 5) + p % 7 for p in every}, True),
    }


MAX_CELLS = 64 << 20   # tokenize_windows: windows x (buckets + 1)
PIECE_CUT = 777        # the input "priors" in two pieces: rows in front of this one, and the rest
