"""-m gpu: the order stage (scalce_batch_order: spill chunks, radix passes of prims.hpp, run_small_sort_k and its way out) and
the emit stage (emit_reads_k in both layouts, gather_rows_k) at their own edges.

The reference of every comparison is the oracle: Trie.tokenize / Trie.order for tokens and permutation, orc_cli's files for
the bytes of .scalcer, .scalcen and .scalceq.  Inputs are crafted, and every test proves from the oracle's tokens that its
input is what it claims -- run lengths on (bucket, chunk, 16-base prefix), where the runs lie, which `end` values occur,
which workgroups are staged -- before the device is consulted; the path the device took is asserted from
scalce_batch_stats (chunks, order_run_members, order_radix_fallback) and the fused flag.

Two constructions.  The tokenizer takes the longest core of a read (N counts as A there as everywhere), among equally long
ones the one whose bucket is fuller, so:
  * a read without any core -- random bases, changed one at a time wherever the oracle still finds one -- lies in the root
    bucket with end = 0, and its key is its first 16 bases; the root comes last in the order;
  * a read with ONE core of 12 bases, the table's longest, and 16 chosen bases behind it lies in that core's bucket with a
    key of the test's choosing, whatever shorter cores it holds by chance.
Either way the oracle's tokens have the last word: the builders change free bases until every row is what was planned.
"""
import functools
import os
import re

import numpy as np
import pytest

import oraclelib as O
from gpu_util import (PREFIX_BASES, RUN_SMALL_MAX, chunks_by_rule, device_bytes, key16, order_expectation, record_sizes)
from scalce_amd import format as fmt
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
PBIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patterns.bin")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
WG = 256                       # threads of emit_reads_k / run_small_sort_k workgroups
EMIT_STAGE_BYTES = 256 * 64    # kernels_order.hpp
HEADER = 12                    # [int32 core][int64 count] in front of a bucket's records


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


@functools.lru_cache(maxsize=None)
def table():
    """(oracle trie, length of every core, the cores as uint8 arrays)"""
    trie = O.Trie(blob=open(PBIN, "rb").read())
    lens = trie.pattern_lens()
    cores = [np.frombuffer(trie.pattern(p), dtype=np.uint8) for p in range(trie.n_patterns)]
    assert lens.min() == 8 and all(len(c) == n for c, n in zip(cores, lens))
    return trie, lens, cores


def random_rows(rng, n, L):
    return ACGT[rng.integers(0, 4, size=(n, L))]


def change_base(rng, rows, r, j):
    rows[r, j] = ACGT[(int(np.flatnonzero(ACGT == rows[r, j])[0]) + int(rng.integers(1, 4))) % 4]


def coreless(rng, n, L):
    """random reads in which the oracle finds no core: one base of every core found is changed until none is left"""
    trie, lens, _ = table()
    rows = random_rows(rng, n, L)
    while True:
        pat, end = trie.tokenize(rows)
        bad = np.flatnonzero(pat >= 0)
        if not len(bad):
            return rows
        for r in bad:
            change_base(rng, rows, r, int(end[r]) - 1 - int(rng.integers(0, lens[pat[r]])))


def fastq(bases, seed, prefix="s.", suffix=""):
    rng = np.random.default_rng(seed)
    quals = (np.clip(np.rint(rng.normal(30.0, 8.0, size=bases.shape)), 2, 40) + 33).astype(np.uint8)
    return synth.fastq_bytes_fast(bases, quals, prefix=prefix, suffix=suffix)


def name_lens(n, prefix="s.", suffix=""):
    return np.array([len(prefix) + len(str(i)) + len(suffix) for i in range(n)], dtype=np.int64)


# ---- device and oracle runs ----------------------------------------------------------------------------------------------
def device_run(ctx, fq1, L, fq2=None, L2=0, B=0, fused=None, coder=True, qmap=None):
    """One batch through every stage (coder=False: up to the emit stage).  fused: True / False asks for that row layout --
    set_fused_rows raises when the batch cannot take it, which is how the tests assert the layout -- None leaves it."""
    t1 = device_bytes(fq1)
    t2 = device_bytes(fq2) if fq2 is not None else None
    n = fq1.count(b"\n") // 4
    b = host.Batch(ctx, L, n + 8, max(len(fq1), len(fq2 or b"")) + 64, paired=fq2 is not None, read_len2=L2, qmap=qmap,
                   bucket_set_size=B)
    if fused is not None:
        b.set_fused_rows(fused)
    run = b.compress if coder else b.front
    run(t1.data_ptr(), len(fq1), t2.data_ptr() if t2 is not None else None, len(fq2 or b""))
    b.finish()
    b._keep = (t1, t2)
    return b


class View:
    """what the oracle says about an input: tokens, spill chunks by the -B rule, permutation, and the runs of the order"""

    def __init__(self, bases, B=0):
        trie, lens, _ = table()
        self.bases = bases
        self.n, self.L = bases.shape
        self.pat, self.end = trie.tokenize(bases)
        self.chunk, self.nchunks = None, 1
        if B:
            sz = record_sizes(self.pat, lens, name_lens(self.n), self.L)
            self.chunk, self.nchunks = chunks_by_rule(sz, B)
        self.perm = trie.order(bases, self.pat, self.end, self.chunk if self.nchunks > 1 else None)
        self.members, self.fallback, self.starts, self.lens = order_expectation(bases, self.pat, self.end, self.perm, self.chunk)

    def run_at(self, pos):
        """(first position, length) of the run that holds position `pos` of the permutation"""
        k = int(np.searchsorted(self.starts, pos, side="right")) - 1
        return int(self.starts[k]), int(self.lens[k])

    def reordered(self, start, n):
        """phase 1 leaves a run in input order: phase 2 has work to do when the oracle's order of it is another"""
        return bool((np.diff(self.perm[start:start + n]) < 0).any())


def check_order(ctx, view, monkeypatch, B=0, seed=1):
    """tokens, permutation and the path taken against the oracle's view; then the all-digits sort: same permutation"""
    fq = fastq(view.bases, seed)
    b = device_run(ctx, fq, view.L, B=B, coder=False)
    st = b.stats()
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    assert (tok[:, 0] == view.pat).all() and (tok[:, 1] == view.end).all(), "tokens differ from the oracle's"
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    bad = np.flatnonzero(perm != view.perm)
    assert len(bad) == 0, f"permutation differs at {len(bad)} of {view.n} positions, first {bad[:5]} ({st})"
    assert st["chunks"] == view.nchunks
    assert st["order_run_members"] == view.members, (st, view.members)
    assert (st["order_radix_fallback"] != 0) == view.fallback, (st, view.fallback)
    monkeypatch.setenv("SCALCE_ORDER_SINGLE_PHASE", "1")
    try:
        b2 = device_run(ctx, fq, view.L, B=B, coder=False)
    finally:
        monkeypatch.delenv("SCALCE_ORDER_SINGLE_PHASE")
    st2 = b2.stats()
    assert st2["order_run_members"] == 0 and st2["order_radix_fallback"] == 0 and st2["chunks"] == view.nchunks
    assert (b2.output(host.OUT_PERM, 0, np.uint32) == view.perm).all(), "the all-digits sort gives another permutation"
    return b, st


def check_files(ctx, d, fq1, L, fq2=None, L2=0, B=0, fused=None, tag="x"):
    """.scalce{r,n,q} of every mate, written from the batch by format.write_archive, against orc_cli's; -> (batch, the
    chunk count orc_cli reports)"""
    d = str(d)
    in1 = os.path.join(d, f"{tag}_1.fq")
    open(in1, "wb").write(fq1)
    off, vals, _ = fmt.sample_qmap(fq1)
    qm = [(off, vals), (off, vals)]
    flags = ["-v"] + (["-B", str(B)] if B else [])
    if fq2 is not None:
        open(os.path.join(d, f"{tag}_2.fq"), "wb").write(fq2)
        qm[1] = fmt.sample_qmap(fq2)[:2]
        flags.append("-r")
    r = O.orc_cli("compress", PBIN, in1, os.path.join(d, tag + "_orc"), *flags)
    nrec, nchunks = map(int, re.search(rb"oracle: (\d+) reads, (\d+) chunk", r.stderr).groups())
    assert nrec == fq1.count(b"\n") // 4
    b = device_run(ctx, fq1, L, fq2=fq2, L2=L2, B=B, fused=fused, qmap=qm)
    fmt.write_archive(os.path.join(d, tag + "_hip"), b, off)
    compare_archives(d, tag, 2 if fq2 is not None else 1)
    return b, nchunks


def compare_archives(d, tag, mates, what=""):
    for m in range(1, mates + 1):
        for ext in "rnq":
            a = open(os.path.join(d, f"{tag}_orc_{m}.scalce{ext}"), "rb").read()
            h = open(os.path.join(d, f"{tag}_hip_{m}.scalce{ext}"), "rb").read()
            assert len(a) == len(h), f"{what}{tag} .scalce{ext} mate {m}: {len(h)} bytes, the oracle's {len(a)}"
            if a != h:
                at = int(np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(h, np.uint8))[0])
                raise AssertionError(f"{what}{tag} .scalce{ext} mate {m} differs first at byte {at} of {len(a)}")


# ---- crafted inputs for the order stage ----------------------------------------------------------------------------------
# A segment is a stretch of the final order inside one of two buckets -- one core's, and the root's, which comes last.  Its
# place follows from its key: the first three bases of the key count the segments up.
def rank3(k):
    assert 0 <= k < 64
    return ACGT[[(k >> 4) & 3, (k >> 2) & 3, k & 3]]


def core_rows(rng, L, core, rank, members, single=False):
    """Rows of the core's bucket.  members[i] = bases behind the core of row i: up to 16 lie inside the prefix (the row's key
    is over there: nothing is left to sort it by), more leave `t - 16` random bases behind it.  The rows of a run share
    the key rank | 7 bases | AAAAAA -- so a core ending 10, 12, 16, 20 or 40 bases before the read's end gives the same 16
    padded bases -- and differ in `end`; single: every row a key of its own (13 random bases behind the rank).
    -> (rows, the bases that may still change: those in front of the core and behind the key)"""
    rows = random_rows(rng, len(members), L)
    free = np.ones(rows.shape, dtype=bool)
    K = np.concatenate([rank3(rank), ACGT[rng.integers(0, 4, size=7)], ACGT[np.zeros(6, dtype=np.int64)]])
    for i, t in enumerate(members):
        if single:
            K = np.concatenate([rank3(rank), ACGT[rng.integers(0, 4, size=13)]])
        e = L - t
        rows[i, e - len(core):e] = core
        rows[i, e:e + min(t, PREFIX_BASES)] = K[:t]
        free[i, e - len(core):e + PREFIX_BASES] = False
    return rows, free


def root_rows(rng, L, rank, n, single=False):
    """Rows of the root bucket (no core, end = 0): a run shares its first 16 bases and differs behind them"""
    rows = random_rows(rng, n, L)
    free = np.ones(rows.shape, dtype=bool)
    rows[:, :3] = rank3(rank)
    free[:, :3] = False
    if not single:
        rows[:, 3:PREFIX_BASES] = rows[0, 3:PREFIX_BASES]
        rows[:, PREFIX_BASES] = ACGT[3 - (np.arange(n) * 4) // n]   # the later in the input, the smaller: there is sorting to do
        free[:, :PREFIX_BASES + 1] = False
    return rows, free


MIX = (40, 10, 20, 16, 12, 24, 16, 33)   # bases behind the core, cycled through the members of a run that needs sorting:
                                         # the first member has bases behind the prefix, the second none, so it sorts in front
INSIDE = (10, 16, 12, 14, 11, 16, 13)    # ... of a run whose members all end inside the prefix


def mix(n, kinds=MIX):
    return [kinds[i % len(kinds)] for i in range(n)]


def build_order_input(seed, core_segments, root_segments, L=100):
    """core_segments: lists of `members` (a run) or ints (that many singles), in the order they are to stand in the core's
    bucket; root_segments: ints -- n > 0 a run of n, n < 0 that many singles.  The rows are dealt over the input at random;
    the members of a run keep their order (the i-th member is the i-th of them in the input, so also the i-th behind phase 1).
    Free bases are changed until the oracle's tokens confirm every row.  -> (View, input row of every planned row)"""
    trie, lens, cores = table()
    longest = np.flatnonzero(lens == lens.max())
    for attempt in range(50):
        rng = np.random.default_rng([seed, attempt])
        p = int(longest[rng.integers(0, len(longest))])
        parts, want_end = [], []
        for k, seg in enumerate(core_segments):
            members = mix(seg, (40, 36, 29)) if isinstance(seg, int) else list(seg)
            parts.append(core_rows(rng, L, cores[p], k, members, single=isinstance(seg, int)))
            want_end += [L - t for t in members]
        ncore = len(want_end)
        for k, seg in enumerate(root_segments):
            parts.append(root_rows(rng, L, k, abs(seg), single=seg < 0))
            want_end += [0] * abs(seg)
        n = len(want_end)
        where = rng.permutation(n)
        at, pos = 0, np.empty(n, dtype=np.int64)
        for rows, _ in parts:   # a segment's rows go to the places dealt to it, in their own order
            pos[at:at + len(rows)] = np.sort(where[at:at + len(rows)])
            at += len(rows)
        bases = np.empty((n, L), dtype=np.uint8)
        free = np.empty((n, L), dtype=bool)
        bases[pos] = np.concatenate([rows for rows, _ in parts])
        free[pos] = np.concatenate([f for _, f in parts])
        want_pat = np.full(n, -1, dtype=np.int32)
        want_pat[pos[:ncore]] = p
        end = np.empty(n, dtype=np.int32)
        end[pos] = want_end
        for _ in range(200):
            pat, got_end = trie.tokenize(bases)
            bad = np.flatnonzero((pat != want_pat) | (got_end != end))
            if not len(bad):
                return View(bases), pos
            stuck = False
            for r in bad:   # the core found instead: one of its free bases becomes another
                cand = np.flatnonzero(free[r, got_end[r] - lens[pat[r]]:got_end[r]]) + got_end[r] - lens[pat[r]] if pat[r] >= 0 else []
                if not len(cand):
                    stuck = True   # (it lies in the planned bases: another draw)
                    break
                change_base(rng, bases, r, int(cand[rng.integers(0, len(cand))]))
            if stuck:
                break
    raise AssertionError("no draw whose tokens are the planned ones: take another seed")


def segment_start(core_segments, root_segments, k, root=False):
    sizes = [s if isinstance(s, int) else len(s) for s in core_segments] + [abs(s) for s in root_segments]
    return sum(sizes[:k + (len(core_segments) if root else 0)])


# ---- run lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 34, 64, 65, 2049])
def test_run_lengths_at_the_ends_and_across_a_workgroup_edge(n, ctx, monkeypatch):
    """A run of n records that need sorting -- their `end` values differ, their keys agree on the padded prefix -- three
    times in one batch: at position 0 of the permutation, on the last positions (root bucket), and in between across two
    workgroup edges at once.  Its middle is a multiple of 256 in POSITIONS, the edge of run_heads_keys_k and run_compact_k,
    which look at the neighbour's head across it; and -- by small runs of up to 32 in front of it -- a multiple of 256 in
    the RANK among the run members, the edge of run_small_sort_k, which is indexed by that rank.  2049 is one more than a
    radix tile.  Up to 32 the runs are sorted where they stand; from 33 on everything goes through the radix passes."""
    half = (n + 1) // 2
    first = ((n + half) // WG + 2) * WG - half      # where the second run begins: its middle is a multiple of 256
    fill = (-((n if n > 1 else 0) + half)) % WG     # run members to put in front of it so that its middle is one by rank as well
    fill += WG if fill < 2 else 0
    small = [32] * (fill // 32) + ([fill % 32] if fill % 32 else [])
    if small[-1] == 1:                              # (no run of one)
        small[-2:] = [small[-2] - 1, 2] if len(small) > 1 else [fill]
    assert sum(small) == fill and min(small) >= 2 and max(small) <= RUN_SMALL_MAX
    core_segments = [mix(n)] + [mix(k) for k in small] + [first - n - fill, mix(n), 37]
    root_segments = [-40, n]
    v, _ = build_order_input(100 + n, core_segments, root_segments)
    total = v.n
    assert total == first + n + 37 + 40 + n
    member = np.repeat(v.lens > 1, v.lens)          # by position: in a run of two or more
    rank = int(member[:first].sum())                # what run_compact_k numbers the second run's first member
    assert (rank + half) % WG == 0 and (n == 1 or rank // WG != (rank + n - 1) // WG)
    for start, what in ((0, "at position 0"), (first, "across a workgroup edge"), (total - n, "on the last positions")):
        assert v.run_at(start) == (start, n), f"the run of {n} {what} is not there: {v.run_at(start)}"
        if n > 1:
            assert v.reordered(start, n), f"the run {what} is in its final order already"
    if n > 1:
        assert first // WG != (first + n - 1) // WG and (first + (n + 1) // 2) % WG == 0
        assert len(set(v.end[v.perm[:n]])) >= min(n, 4), "the members of a run in the core's bucket differ in `end`"
    assert v.lens.max() == max(n, max(small)) and v.fallback == (n > RUN_SMALL_MAX)
    assert v.members == (3 * n if n > 1 else 0) + fill
    check_order(ctx, v, monkeypatch)


SMALL_CORE = [mix(2), 3, mix(3), 5, mix(31), 2, mix(32), 200, mix(5), 30]
SMALL_ROOT = [-20, 32, -3, 2, -250, 7]


def test_only_small_runs_are_sorted_where_they_stand(ctx, monkeypatch):
    """(i) runs of 2 .. 32 that need sorting and nothing longer: no radix pass behind run_small_sort_k"""
    v, _ = build_order_input(1, SMALL_CORE, SMALL_ROOT)
    assert sorted(v.lens[v.lens > 1]) == [2, 2, 3, 5, 7, 31, 32, 32] and not v.fallback
    assert all(v.reordered(s, n) for s, n in zip(v.starts, v.lens) if n > 2)
    _, st = check_order(ctx, v, monkeypatch)
    assert st["order_radix_fallback"] == 0 and st["order_run_members"] == 114


def test_one_run_of_33_sends_everything_through_the_passes(ctx, monkeypatch):
    """(ii) the same small runs -- sorted where they stand first -- and ONE run of 33 with bases behind the prefix: the
    radix passes then take every run again, the sorted small ones included"""
    v, _ = build_order_input(2, SMALL_CORE, SMALL_ROOT + [-4, 33])
    assert sorted(v.lens[v.lens > 1]) == [2, 2, 3, 5, 7, 31, 32, 32, 33] and v.fallback
    assert v.run_at(v.n - 1) == (v.n - 33, 33) and v.reordered(v.n - 33, 33)
    _, st = check_order(ctx, v, monkeypatch)
    assert st["order_radix_fallback"] != 0 and st["order_run_members"] == 147


def test_long_runs_that_end_inside_the_prefix_stay_as_they_are(ctx, monkeypatch):
    """(iii) runs of 33 .. 300 whose members all end within the prefix (end + 16 >= L: nothing is left to sort them by)
    beside small runs that need sorting: no way out through the passes, the long runs keep their input order"""
    core_segments = [mix(33, INSIDE), 7, mix(6), mix(300, INSIDE), 100, mix(34, INSIDE), mix(30), 3, mix(65, INSIDE)]
    v, _ = build_order_input(3, core_segments, [-10, 9, -5])
    long_runs = [(s, n) for s, n in zip(v.starts, v.lens) if n > RUN_SMALL_MAX]
    assert sorted(n for _, n in long_runs) == [33, 34, 65, 300] and not v.fallback
    for s, n in long_runs:
        members = v.perm[s:s + n]
        assert (v.end[members] + PREFIX_BASES >= v.L).all() and len(set(v.end[members])) > 3
        assert not v.reordered(s, n)
    assert sorted(n for n in v.lens if 1 < n <= RUN_SMALL_MAX) == [6, 9, 30]
    assert all(v.reordered(s, n) for s, n in zip(v.starts, v.lens) if 1 < n <= RUN_SMALL_MAX)
    _, st = check_order(ctx, v, monkeypatch)
    assert st["order_radix_fallback"] == 0


@pytest.mark.parametrize("behind", [(39, 69), (10,), (69,), (0,)], ids=["40th_and_last", "11th", "last", "head"])
def test_a_long_run_with_one_member_behind_the_prefix(behind, ctx, monkeypatch):
    """(iv) a run of 70 in which only the named members (in input order, which is their order behind phase 1) have bases
    behind the prefix.  The head's thread sees a long run and, unless it is the head itself, nothing to sort; the flag has
    to come from the member's own thread, which finds the run long by looking up to 32 places back (the 40th, the last) or
    forth (the 11th).  The member sorts behind all the others."""
    members = mix(70, INSIDE)
    for i in behind:
        members[i] = 20
    v, pos = build_order_input(40 + sum(behind), [5, members, 9, mix(3)], [-6, 4])
    s, n = v.run_at(5)
    assert (s, n) == (5, 70) and v.fallback
    run_rows = np.sort(v.perm[s:s + n])       # the run's members in input order
    assert tuple(np.flatnonzero(v.end[run_rows] + PREFIX_BASES < v.L)) == behind
    assert (v.end[v.perm[s + n - len(behind):s + n]] == v.L - 20).all(), "the members with bases behind the prefix come last"
    assert v.lens.max() == 70
    _, st = check_order(ctx, v, monkeypatch)
    assert st["order_radix_fallback"] != 0


@pytest.mark.parametrize("longest", [32, 40])
def test_whole_read_duplicates_keep_their_input_order(longest, ctx, monkeypatch, tmp_path):
    """(v) whole-read duplicates with names and qualities of their own: equal keys keep the input order through the
    insertion sort (strictly less) and through the radix passes (longest = 40 takes them) -- it shows in .scalcen and
    .scalceq, compared with the oracle's files -- and through the all-digits index passes."""
    core_segments = [mix(2), 4, mix(longest), 10, mix(7)]
    root_segments = [-5, 12, -3, 3]
    v, pos = build_order_input(60 + longest, core_segments, root_segments)
    bases = v.bases.copy()
    at = 0
    for seg in core_segments + root_segments:   # every run becomes copies of its first and its last row, turn by turn
        n = abs(seg) if isinstance(seg, int) else len(seg)
        if not isinstance(seg, int) or (seg > 0 and at >= segment_start(core_segments, root_segments, 0, root=True)):
            rows = pos[at:at + n]
            bases[rows] = bases[rows[[0, n - 1]]][np.arange(n) % 2]
        at += n
    v = View(bases)
    assert sorted(v.lens[v.lens > 1]) == sorted([2, 7, longest, 12, 3]) and v.fallback == (longest > RUN_SMALL_MAX)
    for s, n in zip(v.starts, v.lens):
        if n > 1:   # two reads, many copies of each: copies keep their input order
            assert len(np.unique(bases[v.perm[s:s + n]], axis=0)) == 2
            assert n < 3 or v.reordered(s, n)
    check_order(ctx, v, monkeypatch, seed=5)
    b, _ = check_files(ctx, tmp_path, fastq(bases, 5), v.L)
    st = b.stats()
    assert (b.output(host.OUT_PERM, 0, np.uint32) == v.perm).all()
    assert st["order_run_members"] == v.members and (st["order_radix_fallback"] != 0) == v.fallback


# ---- spill chunks ------------------------------------------------------------------------------------------------------
def limit_for(sizes, nchunks):
    """a -B that cuts this input into exactly `nchunks` chunks by the rule"""
    total = int(sizes.sum())
    if nchunks == 1:
        return total + 1
    for B in range(total // nchunks + 1, total // (nchunks - 1) + 2):
        if chunks_by_rule(sizes, B)[1] == nchunks:
            return B
    raise AssertionError(f"no -B cuts the input into {nchunks} chunks")


def chunked_input(nchunks):
    """Runs that phase 2 reorders, dealt over the whole input (so every chunk holds parts of most of them), and an exact
    duplicate on both sides of every chunk boundary.  -> (View with the chunks of its -B, that -B)"""
    trie, lens, _ = table()
    core_segments = [x for k in range(30) for x in (mix(12 + k % 9), 20)]
    v, _ = build_order_input(7, core_segments, [-30, 25, -30, 40, -10])
    bases = v.bases.copy()
    k = 0
    while True:   # a boundary follows from the rows in front of it alone: making row r a copy of row r - 1 leaves it where it is
        pat, _ = trie.tokenize(bases)
        sizes = record_sizes(pat, lens, name_lens(len(bases)), v.L)
        B = limit_for(sizes, nchunks)
        cuts = np.flatnonzero(np.diff(chunks_by_rule(sizes, B)[0])) + 1
        if k >= len(cuts):
            break
        bases[cuts[k]] = bases[cuts[k] - 1]
        k += 1
    v = View(bases, B=B)
    assert v.nchunks == nchunks
    return v, B


def end_in_key_chunks(n_patterns):
    """the largest chunk count at which `end` still rides in the sort key: 16 + PREFIX_BITS + cbits + bits <= 64"""
    bits = 1
    while (1 << bits) < n_patterns + 1:
        bits += 1
    return 1 << (64 - 16 - 2 * PREFIX_BASES - bits)


@pytest.mark.parametrize("which", ["one", "two", "end_in_key_most", "end_through_perm_least"])
def test_chunk_counts_around_the_end_bits_switch(which, ctx, monkeypatch, tmp_path):
    """1 chunk (-B larger than the input), 2, and the two counts on either side of the switch between `end` carried in the
    key's low bits (rewritten when phase 2 moves a record) and `end` gathered through the permutation -- 4 and 5 for the
    shipped table, derived from its size.  The runs are reordered by phase 2 and their members differ in `end`, so an
    `end` that stayed behind shows in .scalcer; duplicates that straddle a chunk boundary are no run."""
    assert ctx.n_buckets == ctx.n_patterns
    most = end_in_key_chunks(ctx.n_patterns)
    assert 2 < most < 64
    nchunks = {"one": 1, "two": 2, "end_in_key_most": most, "end_through_perm_least": most + 1}[which]
    v, B = chunked_input(nchunks)
    cuts = np.flatnonzero(np.diff(v.chunk)) + 1 if v.chunk is not None else []
    assert len(cuts) == nchunks - 1
    for r in cuts:
        assert (v.bases[r] == v.bases[r - 1]).all() and v.chunk[r] != v.chunk[r - 1]
        kr, k1 = int(np.flatnonzero(v.perm == r)[0]), int(np.flatnonzero(v.perm == r - 1)[0])
        assert v.run_at(kr)[0] != v.run_at(k1)[0], "duplicates in two chunks are in one run"
    moved = [(s, n) for s, n in zip(v.starts, v.lens) if n > 1 and v.reordered(s, n) and len(set(v.end[v.perm[s:s + n]])) > 1]
    assert len(moved) >= 20, "runs that phase 2 reorders and whose members differ in `end`"
    check_order(ctx, v, monkeypatch, B=B)
    b, orc_chunks = check_files(ctx, tmp_path, fastq(v.bases, 1), v.L, B=B)
    assert b.stats()["chunks"] == orc_chunks == nchunks


@functools.lru_cache(maxsize=None)
def synth_30000():
    return synth.reads_and_quals(30000, 100, seed=21, n_frac=0.004, dup_frac=0.15)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 9000])
def test_every_record_a_chunk(n, ctx, monkeypatch, tmp_path):
    """-B 1: n chunks of one record, on both sides of 4096 and far beyond.  Neighbours that are exact duplicates are in
    different chunks: there is no run at all, every bucket keeps its input order."""
    bases, quals = (x[:n].copy() for x in synth_30000())
    bases[1::50] = bases[0::50][:len(bases[1::50])]
    v = View(bases, B=1)
    assert v.nchunks == n and (v.chunk == np.arange(n)).all() and v.members == 0
    check_order(ctx, v, monkeypatch, B=1)
    b, orc_chunks = check_files(ctx, tmp_path, synth.fastq_bytes_fast(bases, quals), 100, B=1)
    assert b.stats()["chunks"] == orc_chunks == n


def test_five_thousand_chunks(ctx, monkeypatch, tmp_path):
    """-B 1000 on 30 000 reads of 100 bp: 5000 chunks of six records"""
    bases, quals = synth_30000()
    v = View(bases, B=1000)
    assert v.nchunks == 5000
    check_order(ctx, v, monkeypatch, B=1000)
    b, orc_chunks = check_files(ctx, tmp_path, synth.fastq_bytes_fast(bases, quals), 100, B=1000)
    assert b.stats()["chunks"] == orc_chunks == 5000


def test_five_thousand_chunks_through_the_streaming_entry(ctx, tmp_path):
    """The same through scalce_stream_compress, the entry the `scalce` binary drives (its own -B takes whole megabytes, as
    the reference's does: 5000 chunks of those are gigabytes of input): pieces of 300 KB, chunks cut on run-wide sizes."""
    import ctypes as C
    bases, quals = synth_30000()
    fq = synth.fastq_bytes_fast(bases, quals)
    open(tmp_path / "s_1.fq", "wb").write(fq)
    r = O.orc_cli("compress", PBIN, tmp_path / "s_1.fq", tmp_path / "s_orc", "-v", "-B", "1000")
    assert b"30000 reads, 5000 chunk(s)" in r.stderr
    off, vals, _ = fmt.sample_qmap(fq)
    p = host.Params()
    host.lib().scalce_params_default(C.byref(p))
    p.read_len[0], p.bucket_set_size = 100, 1000
    for m in range(2):
        p.qmap[m].offset = int(off)
        for i in range(128):
            p.qmap[m].values[i] = int(vals[i])
    pos = [0]

    def rd(cap):
        k = min(cap, len(fq) - pos[0])
        pos[0] += k
        return fq[pos[0] - k:pos[0]]
    b, st = host.stream_compress(ctx, p, rd, None, piece_bytes=300_000)
    assert b.n_reads == 30000 and st.rounds > 5 and b.stats()["chunks"] == 5000
    fmt.write_archive(str(tmp_path / "s_hip"), b, off)
    compare_archives(str(tmp_path), "s", 1)


# ---- emit: records of every `end`, every layout, both ways out of a workgroup ------------------------------------------
def emit_input(L, n, seed, distinct=False):
    """Rows whose planned `end` cycles through 0 (no core), a core at base 0, a core on the last base, and every value in
    between from 9 up: the first 19 rows hold every residue modulo 16 already.  distinct: no core twice."""
    _, lens, cores = table()
    rng = np.random.default_rng([L, seed])
    rows = coreless(rng, n, L)
    targets = [0, -1, L] + list(range(9, L))
    deck = iter(rng.permutation(len(cores)))
    for i in range(n):
        e = targets[i % len(targets)]
        if e == 0:
            continue
        while True:
            core = cores[int(next(deck)) if distinct else int(rng.integers(0, len(cores)))]
            if len(core) <= (e if e > 0 else L):
                break
        e = len(core) if e < 0 else e
        rows[i, e - len(core):e] = core
    return rows


def assert_every_end(pat, end, L):
    _, lens, _ = table()
    level = np.where(pat >= 0, lens[np.maximum(pat, 0)], 0)
    assert ((pat < 0) & (end == 0)).any(), "no read without a core"
    assert ((pat >= 0) & (end == level)).any(), "no core at base 0"
    assert ((pat >= 0) & (end == L)).any(), "no core on the last base"
    between = end[(pat >= 0) & (end > level) & (end < L)]
    assert {int(e) % 16 for e in between} == {e % 16 for e in range(9, L)}, "an offset inside a 32-bit word is missing"


def workgroup_spans(pat, perm, L):
    """bytes of .scalcer every workgroup of emit_reads_k covers (the headers of the buckets that begin in it included),
    its records and the buckets among them -- from the oracle's order"""
    _, lens, _ = table()
    p = pat[np.asarray(perm, dtype=np.int64)]
    level = np.where(p >= 0, lens[np.maximum(p, 0)], 0)
    rec = (L - level + 3) // 4 + (2 if L > 255 else 1)
    first = np.concatenate([[True], p[1:] != p[:-1]])
    cost = rec + HEADER * first
    out = []
    for k0 in range(0, len(p), WG):
        out.append((int(cost[k0:k0 + WG].sum()), len(p[k0:k0 + WG]), len(set(p[k0:k0 + WG]))))
    return out


def is_fused(L):
    return L % 4 == 0 and 16 <= L <= 160   # single-end with qualities: host_state.inc, batch_create


FUSED = [16, 20, 32, 36, 64, 100, 128, 156, 160]
PLAIN = [17, 31, 33, 75, 127, 161, 164, 220, 255, 256, 257, 300]


@pytest.mark.parametrize("L", FUSED + PLAIN)
def test_records_of_every_end_at_every_length(L, ctx, tmp_path):
    """Every length against the oracle's files: N = 1, 255, 256, 257 and 3001 (partial last workgroups), at the fused
    lengths in both row layouts -- which therefore write the same bytes.  Beyond 255 bases the end marker has two bytes,
    and the batch of 3001 takes both ways out: full workgroups of distinct buckets write their records directly, the
    partial last one is staged."""
    assert is_fused(L) == (L in FUSED)
    rows = emit_input(L, 3001, 1)
    trie, lens, _ = table()
    pat, end = trie.tokenize(rows[:40])
    inner = int(np.flatnonzero((pat >= 0) & (end > lens[np.maximum(pat, 0)]) & (end < L))[0])   # a core inside the read
    for n in (3001, 257, 256, 255, 1):
        bases = rows[:n] if n > 1 else rows[inner:inner + 1]
        pat, end = trie.tokenize(bases)
        if n > 1:
            assert_every_end(pat, end, L)
        else:
            assert pat[0] >= 0 and lens[pat[0]] < end[0] < L
        spans = workgroup_spans(pat, trie.order(bases, pat, end), L)
        staged = {s <= EMIT_STAGE_BYTES for s, _, _ in spans}
        if WG * ((L + 3) // 4 + 2 + HEADER) <= EMIT_STAGE_BYTES:
            assert staged == {True}     # whatever the buckets: 256 records and 256 headers fit the stage
        if n == 3001 and L > 255:
            assert staged == {True, False}, "the two-byte marker takes both ways out"
        fq = fastq(bases, L + n)
        for fused in ((True, False) if is_fused(L) else (None,)):
            check_files(ctx, tmp_path, fq, L, fused=fused, tag=f"n{n}" + {None: "", True: "_fused", False: "_rows"}[fused])
    if not is_fused(L):   # (and the batch says so itself)
        b = host.Batch(ctx, L, 16, 4096)
        with pytest.raises(host.ScalceError):
            b.set_fused_rows(True)


def test_staged_and_direct_workgroups_in_one_batch(ctx, tmp_path):
    """L = 220: a workgroup of 256 records of ONE bucket covers 256 x 56 bytes and a header and is staged in LDS; one of
    256 records of 256 buckets, each with its header, is over EMIT_STAGE_BYTES and writes directly.  Both in one batch."""
    L = 220
    one_bucket = WG * ((L + 3) // 4 + 1) + HEADER
    all_buckets = WG * ((L - 12 + 3) // 4 + 1 + HEADER)     # (the longest core has 12 bases)
    assert one_bucket <= EMIT_STAGE_BYTES < all_buckets
    rng = np.random.default_rng(220)
    bases = np.concatenate([emit_input(L, 1400, 2, distinct=True), coreless(rng, 900, L)])
    bases = bases[rng.permutation(len(bases))]
    trie, _, _ = table()
    pat, end = trie.tokenize(bases)
    assert_every_end(pat, end, L)
    spans = workgroup_spans(pat, trie.order(bases, pat, end), L)
    assert any(s <= EMIT_STAGE_BYTES and n == WG and nb == 1 for s, n, nb in spans), "no staged workgroup of one bucket"
    assert any(s > EMIT_STAGE_BYTES and n == WG and nb >= 250 for s, n, nb in spans), "no direct workgroup of 256 buckets"
    check_files(ctx, tmp_path, fastq(bases, 220), L)


def gather_paths(L1, L2, counts):
    """(whole words per row or not, a tail of fewer than 16 bytes or not) of every gather_rows_k launch of a paired batch:
    mate 2's packed rows (their stride is a multiple of 16) and the q' of both mates (stride = width)"""
    return {("words" if width % 4 == 0 else "bytes", "tail" if (n * width) % 16 else "whole")
            for n in counts for width in ((L2 + 3) // 4, L1, L2)}


GATHER = [(100, 64), (100, 128), (100, 75), (100, 150), (100, 80), (75, 100)]
COUNTS = (3001, 257, 256)


@pytest.mark.parametrize("L1,L2", GATHER, ids=[f"{a}_{b}" for a, b in GATHER])
def test_paired_rows_through_every_gather_path(L1, L2, ctx, tmp_path):
    """gather_rows_k moves mate 2's packed rows and both mates' q' into output order.  Rows of whole words (width and stride
    multiples of 4): one 16-byte move inside a row, four 4-byte moves across a row's end, a tail of fewer than 16 bytes when
    N x width is no multiple of 16; any other width: byte by byte, with and without a tail."""
    every = set().union(*(gather_paths(a, b, COUNTS) for a, b in GATHER))
    assert every == {("words", "whole"), ("words", "tail"), ("bytes", "whole"), ("bytes", "tail")}
    packed2 = (L2 + 3) // 4
    assert (packed2 % 4 == 0) == (L2 in (64, 128, 80)) and (L2 % 4 == 0) == (L2 in (64, 128, 80, 100))
    if L2 == 80:
        assert (3001 * packed2) % 16 and packed2 % 4 == 0    # whole words and a tail: mate 2's packed rows
    rows = emit_input(L1, 3001, 3)
    mate2, _ = synth.reads_and_quals(3001, L2, seed=L2, n_frac=0.01)
    for n in COUNTS:
        fq1 = fastq(rows[:n], n, prefix="p.", suffix="/1")
        fq2 = fastq(mate2[:n], n + 1, prefix="p.", suffix="/2")
        check_files(ctx, tmp_path, fq1, L1, fq2=fq2, L2=L2, tag=f"n{n}")
