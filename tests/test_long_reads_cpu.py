"""No device: the inputs of tests/long_reads.py are what they claim to be, by the oracle alone.

The GPU tests of tests/test_gpu_long_reads.py compare the device with the oracle on these inputs; a comparison on an input that
misses the path it was built for passes emptily.  So here, for every case: the oracle's CLI compresses and decompresses it, and
its tokens, ties and order are where the case says they are.  These are conditions on the inputs, met by the reference; where
one fails the input is wrong, not the condition."""
import os
import subprocess

import numpy as np
import pytest

import filecases as F
import long_reads as LR
import oraclelib as O
import varlen_util as V

CRAFTED = (1000, 2498)


def canon(text):
    """the records of a FASTQ text as a sorted list, the quality under an N being the offset character (qualities.cpp:183)"""
    ln = text.split(b"\n")
    assert ln[-1] == b"" and (len(ln) - 1) % 4 == 0
    return sorted((ln[i], ln[i + 1], ln[i + 2], bytes(33 if b == 78 else q for b, q in zip(ln[i + 1], ln[i + 3])))
                  for i in range(0, len(ln) - 1, 4))


def round_trip(d, text, table=None, flags=()):
    """orc_cli compress and decompress with status 0 (orc_cli raises otherwise); the records come back as a multiset"""
    table = [LR.PBIN] if table is None else ["-P", table]
    src = d / "in_1.fq"
    src.write_bytes(text)
    O.orc_cli("compress", *table, src, d / "arc", *flags)
    O.orc_cli("decompress", *table, d / "arc_1.scalcen", d / "back")
    back = (d / "back_1.fastq").read_bytes()
    assert canon(back) == canon(text)
    return back


# ---- genome ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LR.LONG)
def test_genome(L, tmp_path, oracle_trie):
    bases, quals = LR.genome(257, L)
    assert bases.shape == quals.shape == (257, L)
    round_trip(tmp_path, LR.fastq(bases, quals))
    pat, end = oracle_trie.tokenize(bases)
    assert (pat >= 0).sum() > 200 and end.max() > min(L, 300) - 50 and (end <= L).all()
    assert (bases == ord("N")).any() and len(np.unique(bases, axis=0)) < 257       # N and whole-read duplicates are there
    assert 35 <= np.ptp(quals) <= 40


def test_genome_at_the_limit_is_what_the_issue_measured(oracle_trie):
    bases, _ = LR.genome(257, 2498)
    pat, end = oracle_trie.tokenize(bases)
    lens = oracle_trie.pattern_lens()
    assert (pat >= 0).all(), "no read of 2498 bases from this genome is coreless"
    assert (lens[pat] == 12).sum() > 128 and end.min() < 256 and end.max() > 2048


# ---- ends -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (301,) + CRAFTED)
def test_ends(L, tmp_path, oracle_trie):
    bases, quals, targets, coreless = LR.ends(L)
    assert set(targets) >= {12, 255, 256, 257, L - 1, L} and (L < 2498 or set(targets) >= {511, 512, 2047, 2048})
    round_trip(tmp_path, LR.fastq(bases, quals))
    pat, end = oracle_trie.tokenize(bases)
    assert sorted(end[pat >= 0]) == targets, "one read per listed value of `end`"
    assert (pat < 0).sum() == coreless >= 1 and (end[pat < 0] == 0).all()
    assert (oracle_trie.pattern_lens()[pat[pat >= 0]] == 12).all()
    assert len(set(pat[pat >= 0])) == len(targets)        # a core of its own each
    assert LR.filler_for(L) in LR.FILLERS
    assert oracle_trie.tokenize(LR.row(LR.filler_for(L), L)[None, :])[0][0] < 0


# ---- many candidates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", CRAFTED)
def test_many_candidates(L, tmp_path, oracle_trie):
    bases, quals = LR.many_candidates(L)
    assert len(bases) == 16
    round_trip(tmp_path, LR.fastq(bases, quals))
    pat, end = oracle_trie.tokenize(bases)
    assert (pat >= 0).all() and (oracle_trie.pattern_lens()[pat] == 12).all()
    # every read holds L // 12 cores of 12 bases end to end; cores recur between reads, so the counts decide: not every read
    # keeps its first core
    cores = {c for _, c in LR.shipped_table()[2]}
    k = L // 12
    held = [[bases[r, 12 * i:12 * i + 12].tobytes() for i in range(k)] for r in range(16)]
    assert all(len(set(h)) == k and set(h) <= cores for h in held)
    assert len(set(held[0]) & set(held[1])) > k // 2
    assert (end > 12).any(), "a later core of a read wins on the counts of the reads in front"
    for r in range(16):
        assert oracle_trie.pattern(int(pat[r])) == bases[r, end[r] - 12:end[r]].tobytes()
    if L == 2498:
        assert k == 208


# ---- the homopolymer table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["kmer", "anchor"])
def test_homopolymer_table(walk, tmp_path):
    from scalce_amd import host
    text = LR.homopolymer_table(walk)
    assert host.walk_of_table(text, True) == (("kmer", 0) if walk == "kmer" else ("anchor", 8))
    trie = O.Trie(text=text)
    L = 2498
    bases, quals, kinds = LR.homopolymer_reads(L)
    (tmp_path / "p.txt").write_bytes(text)
    round_trip(tmp_path, LR.fastq(bases, quals), table=tmp_path / "p.txt")
    pat, end = trie.tokenize(bases)
    want = LR.homopolymer_expectation(kinds, L)
    got = [(trie.pattern(int(p)).decode(), int(e)) for p, e in zip(pat, end)]
    assert got == want
    assert {e for _, e in want} == {8, L // 2 + 8} and {c for c, _ in want} == set(LR.HOMO_CORES)
    # the candidate slots of a tie read: every position at which one of the two cores ends
    assert 2 * (L // 2 - 7) > 1000


# ---- prefix runs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", CRAFTED)
def test_prefix_runs(L, tmp_path, oracle_trie):
    import gpu_util as G
    bases, quals, group, where = LR.prefix_runs(L)
    round_trip(tmp_path, LR.fastq(bases, quals))
    assert where == ([L - 1] if L < 2498 else [12 + 4 * 601 + 1, L - 1])
    pat, end = oracle_trie.tokenize(bases)
    perm = oracle_trie.order(bases, pat, end)
    key = G.key16(bases, end)
    at = np.empty(len(perm), dtype=np.int64)
    at[perm] = np.arange(len(perm))
    for g, size in enumerate(LR.RUN_SIZES):
        rows = np.flatnonzero(group == g)
        assert len(rows) == size
        assert len(set(pat[rows])) == 1 and pat[rows[0]] >= 0 and (end[rows] == 12).all() and len(set(key[rows])) == 1
        others = np.delete(np.arange(len(bases)), rows)
        assert (bases[rows][:, np.delete(np.arange(L), where)] == bases[rows[0], np.delete(np.arange(L), where)]).all()
        slots = np.sort(at[rows])
        assert (np.diff(slots) == 1).all(), "the oracle's permutation places the group side by side"
        assert len(set(pat[others]) & {pat[rows[0]]}) == 0
        in_order = perm[slots[0]:slots[0] + size]
        # members by the differing bases (A < C < G < T, the earlier position first), duplicates in input order
        code = np.searchsorted(LR.ACGT, bases[in_order][:, where])
        rank = [tuple(c) + (int(r),) for c, r in zip(code.tolist(), in_order)]
        assert rank == sorted(rank)
        assert len({tuple(c) for c in code.tolist()}) < size, "the group holds exact duplicates"
    members, fallback, starts, lens = G.order_expectation(bases, pat, end, perm)
    assert sorted(lens.tolist()) == sorted(LR.RUN_SIZES) and members == sum(LR.RUN_SIZES) and fallback
    assert G.RUN_SMALL_MAX == 32


# ---- variable length, exceptions ------------------------------------------------------------------------------------------
def test_varlen_lengths(tmp_path):
    L = 2498
    lens = LR.varlen_lengths(L)
    assert {0, 1, 15, 16, 17, 255, 256, 257, 2047, 2048, L - 1, L} <= set(lens.tolist()) and lens.max() == L
    var, pad, names = V.texts(L, lens, 5)
    starts = np.cumsum([0] + [len(r) for r in V.records_of(var)])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    round_trip(tmp_path, pad)       # the reference takes the padded twin


def test_exception_patterns(tmp_path):
    import exception_ref as ER
    L = 2498
    bases, quals, at = LR.exception_patterns(L)
    assert at == [0, 2047, 2048, L - 1]
    m = ER.exception_mask(bases, quals)
    assert np.flatnonzero(m[0]).tolist() == at and m[1].all() and m[2].all()
    assert (bases[1] >= ord("a")).all() and (bases[2] == ord("N")).all() and (quals[2] > 33).all()
    assert m[3:].any(axis=1).sum() > 30 and not m[3:].all(axis=1).any()
    src = tmp_path / "in_1.fq"
    src.write_bytes(LR.fastq(bases, quals))
    O.orc_cli("compress", LR.PBIN, src, tmp_path / "arc")                    # (what comes back is the plain text: ER.plain)
    O.orc_cli("decompress", LR.PBIN, tmp_path / "arc_1.scalcen", tmp_path / "back")
    letters, q = ER.plain(bases, quals)
    assert canon((tmp_path / "back_1.fastq").read_bytes()) == canon(LR.fastq(letters, q))


# ---- the limit ------------------------------------------------------------------------------------------------------------
def test_a_read_of_2499_bases_is_refused_by_the_oracle(tmp_path):
    bases, quals = LR.genome(20, 2499, n_frac=0)
    src = tmp_path / "in_1.fq"
    src.write_bytes(LR.fastq(bases, quals))
    r = O.orc_cli("compress", LR.PBIN, src, tmp_path / "arc", check=False)
    assert r.returncode != 0 and b"(ERROR)" in r.stderr
    bases, quals = LR.genome(20, LR.MAX_LENGTH, n_frac=0)
    round_trip(tmp_path, LR.fastq(bases, quals))


@pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")
def test_reference_binary_writes_the_oracles_archive_at_2498(tmp_path):
    bases, quals = LR.genome(257, 2498)
    text = LR.fastq(bases, quals)
    round_trip(tmp_path, text)
    r = subprocess.run([F.REF_FULL, "compress", LR.PBIN, str(tmp_path / "in_1.fq"), str(tmp_path / "ref"), "-T", "1", "-t",
                        str(tmp_path / "tmp_ref")], capture_output=True)
    assert r.returncode == 0, r.stderr[-1500:]
    for ext in "nrq":
        assert F.content(str(tmp_path / ("ref_1.scalce" + ext))) == F.content(str(tmp_path / ("arc_1.scalce" + ext))), ext
    r = subprocess.run([F.REF_FULL, "decompress", LR.PBIN, str(tmp_path / "arc_1.scalcen"), str(tmp_path / "rback"), "-T", "1"],
                       capture_output=True)
    assert r.returncode == 0, r.stderr[-1500:]
    assert (tmp_path / "rback_1.fastq").read_bytes() == (tmp_path / "back_1.fastq").read_bytes()
