"""No GPU: tests/tie_ref.py against the oracle, and the conditions its inputs are built to meet.

test_gpu_tie_break.py compares the device with tie_ref.settle; here settle and candidates are held against the oracle's
trie walk (O.Trie.tokenize: aho_search with cumulative bin_size) on every table and input that file uses, and the inputs
are shown to be what their cases need -- candidate counts of every class, decisions on equal counts, priors that change
decisions, a global-sweep input that needs more sweeps than one look covers.  These are conditions, asserted, so that a
device test cannot pass on an input that misses its target."""
import collections

import numpy as np
import pytest

import oraclelib as O
import tie_ref as T
from scalce_amd import host

SWEEPS_PER_LOOK = 4   # scalce_batch_tokenize_settle: global sweeps enqueued per look at their flags
_TRIE = {}


def trie(t):
    if t.name not in _TRIE:
        _TRIE[t.name] = O.Trie(text=t.blob) if t.text else O.Trie(blob=t.blob)
    return _TRIE[t.name]


def bases_of(reads):
    L = len(reads[0])
    assert all(len(r) == L for r in reads)
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).reshape(len(reads), L)


def oracle_tokens(t, reads):
    pat, end = trie(t).tokenize(bases_of(reads))
    return list(zip(pat.tolist(), end.tolist()))


@pytest.mark.parametrize("name", T.TABLE_NAMES)
def test_tables_select_their_walks(name):
    t = T.table(name)
    assert host.walk_of_table(t.blob, t.text) == t.walk
    assert trie(t).n_patterns == len(t.cores) == len(set(t.cores))
    assert [trie(t).pattern(p).decode() for p in (0, len(t.cores) // 2, len(t.cores) - 1)] == \
        [t.cores[p] for p in (0, len(t.cores) // 2, len(t.cores) - 1)]
    assert len({len(c) for c in t.pool}) == 1 and all(c in t.pattern for c in t.pool)


@pytest.mark.parametrize("name", T.INPUT_NAMES)
def test_reference_equals_oracle(name):
    """pattern and end of every read, zero prior"""
    t, reads, cands = T.input_candidates(name)
    assert all(set(r) <= set("ACGT") for r in reads)
    toks, counts = T.settle(cands)
    want = oracle_tokens(t, reads)
    bad = [r for r in range(len(reads)) if toks[r] != want[r]]
    assert not bad, f"{name}: {len(bad)} of {len(reads)} reads differ, first {bad[:4]}: {[(toks[r], want[r]) for r in bad[:4]]}"
    assert counts == dict(collections.Counter(p for p, _ in want))
    assert sum(counts.values()) == len(reads)


@pytest.mark.parametrize("name", ["walk_t7", "walk_ten", "walk_anchor_k8", "seq_patterns", "seq_all8", "mixed"])
def test_prefix_as_prior(name):
    """the counts of the rows in front, given as prior or as the batch's earlier pieces, reproduce the oracle's walk over
    all rows on the rows behind; without them most tie decisions of those rows come out differently"""
    t, reads, cands = T.input_candidates(name)
    want = oracle_tokens(t, reads)
    for cut in (len(reads) // 2, 1, len(reads) - 1):
        in_front = T.settle(cands[:cut])[1]
        toks, own = T.settle(cands[cut:], prior=in_front)
        assert toks == want[cut:]
        assert own == dict(collections.Counter(p for p, _ in want[cut:]))
        toks, own = T.settle(cands[cut:], fixed=in_front)
        assert toks == want[cut:]
        assert own == dict(collections.Counter(p for p, _ in want))
    cut = len(reads) // 2
    alone = T.settle(cands[cut:])[0]
    ties = [r for r in T.tie_rows(cands) if r >= cut]
    assert sum(alone[r - cut] != want[r] for r in ties) >= len(ties) // 10


def test_priors_input_behind_its_prefix():
    """the input of the prior cases behind the rows its "prefix" prior stands for: one oracle walk over both"""
    t, front, cf = T.input_candidates("priors_prefix")
    _, reads, cands = T.input_candidates("priors")
    want = oracle_tokens(t, front + reads)
    assert T.settle(cands, prior=T.priors_under_test()["prefix"][0])[0] == want[len(front):]


@pytest.mark.parametrize("name", ["walk_t7", "walk_ten", "walk_anchor_k8", "priors"])
def test_candidate_count_classes(name):
    """2, 3, 4, 5, 6, 7 and 8 or more candidates: at least 50 reads each; reads with more hits than candidates among them"""
    t, reads, cands = T.input_candidates(name)
    cls = collections.Counter(min(len(c), 8) for c in cands)
    assert all(cls[k] >= 50 for k in range(2, 9)), cls
    assert max(len(c) for c in cands) > T_SEQ_STAGED and cls[1] >= 50
    more_hits = sum(1 for r, c in zip(reads, cands) if len(c) > 1 and len(T.occurrences(t.index, r)) > len(c))
    assert more_hits >= 50
    if name != "priors":
        assert len(cands[0]) > 1 and len(cands[-1]) > 1   # tie reads on row 0 and on the last row


T_SEQ_STAGED = 6   # TIESEQ_K: candidates tie_sequential_k stages in LDS; a seventh is read from memory


def test_sequential_inputs_reach_past_the_staged_candidates():
    for name in ("seq_patterns", "seq_all8"):
        _, _, cands = T.input_candidates(name)
        cls = collections.Counter(min(len(c), 8) for c in cands)
        assert cls[7] >= 50 and cls[8] >= 50 and cls[2] >= 50, (name, cls)


@pytest.mark.parametrize("name", ["walk_t7", "walk_ten", "walk_anchor_k8", "priors", "two", "mixed", "seq_patterns", "seq_all8"])
def test_decisions_on_equal_counts(name):
    """at least 5 % of the tie decisions meet equal counts: the strict comparison, first candidate keeps the bucket"""
    _, _, cands = T.input_candidates(name)
    eq, ties = T.equal_count_decisions(cands)
    assert ties >= 200 and 20 * eq >= ties, (eq, ties)


def test_priors_change_what_they_must():
    """Priors that add the same to every candidate leave every decision alone (they test the sums, not the rule); the others
    change at least 10 % of the tie decisions.  Under an equal prior and under 2^33 + {5, 6} at least 5 % of the decisions
    still meet equal counts; the prefix and the rank prior pull the counts apart (2 % and 1 % meet equal counts), which is
    what they are for."""
    t, reads, cands = T.input_candidates("priors")
    ties = T.tie_rows(cands)
    base = T.choices(cands)
    priors = T.priors_under_test()
    assert list(priors) == ["none", "zero", "prefix", "equal", "last_ahead", "above_2_33", "root_only", "high_bits"]
    for name, (prior, must_differ) in priors.items():
        got = T.choices(cands, None, prior)
        moved = sum(got[r] != base[r] for r in ties)
        if must_differ:
            assert 10 * moved >= len(ties), (name, moved, len(ties))
        else:
            assert moved == 0, (name, moved)
        if name in ("none", "zero", "equal", "above_2_33", "root_only"):
            eq, n = T.equal_count_decisions(cands, None, prior)
            assert 20 * eq >= n, (name, eq, n)
    # high_bits: kept in 32 bits it would be another prior, one that decides at least 10 % of the tie reads differently
    hb = priors["high_bits"][0]
    low, full = T.choices(cands, None, {q: v & 0xFFFFFFFF for q, v in hb.items()}), T.choices(cands, None, hb)
    assert 10 * sum(low[r] != full[r] for r in ties) >= len(ties) and max(hb.values()) >> 32 == 4
    p = priors["above_2_33"][0]
    assert set(p) == set(range(len(t.cores))) | {T.ROOT} and {v - (1 << 33) for v in p.values()} == {5, 6}
    assert set(priors["equal"][0]) == set(p) and len(set(priors["equal"][0].values())) == 1
    # the rank prior: the cores of a read stand in pool order, so under it a later candidate starts ahead of every
    # earlier one, the last ahead of all -- and the first tie read, which takes its first candidate without a prior, takes its last
    rank = priors["last_ahead"][0]
    out_of_order = sum(1 for c in cands if [rank[q] for q, _ in c] != sorted(rank[q] for q, _ in c))
    assert 50 * out_of_order <= len(cands)   # (a core that occurs by chance, in front of the planted ones: a read in a hundred)
    first = ties[0]
    assert base[first] == 0 and T.choices(cands, None, rank)[first] == len(cands[first]) - 1


def test_two_candidate_input():
    """every tie read holds exactly two cores, 200 of them: W = 32 / 31 / 33 tie reads are 64 / 62 / 66 candidate events, so
    the windows' cells begin on bit 0, on bits 62, 60 .. and on bits 2, 4 .. of the bitmap's words"""
    _, reads, cands = T.input_candidates("two")
    assert set(map(len, cands)) == {1, 2}
    assert len(T.tie_rows(cands)) == 200 and len(reads) > 256


def test_edge_batches():
    n = 300
    for name, want in (("tie_first_only", [0]), ("tie_last_only", [n - 1]), ("no_tie", [])):
        _, reads, cands = T.input_candidates(name)
        assert len(reads) == n and T.tie_rows(cands) == want and all(len(c) >= 1 for c in cands)


def test_global_sweep_input_outlasts_one_look():
    """a read of B, then 16 reads "A then B": sweeps settle 1, 2, 4, 8 and 1 reads, and a sixth moves nothing"""
    _, reads, cands = T.input_candidates("doubling")
    assert len(reads) == 17 and T.jacobi_sweeps(cands) == 6 > SWEEPS_PER_LOOK
    assert T.choices(cands) == [0] + [1] * 16
    for name in ("walk_ten", "seq_patterns", "seq_all8"):   # the other inputs that go through the global sweeps' way out
        assert T.jacobi_sweeps(T.input_candidates(name)[2]) > SWEEPS_PER_LOOK
    # the simulation's fixed point is the sequential rule's
    assert T.jacobi_sweeps([[(0, 5), (1, 9)], [(0, 5), (1, 9)], [(1, 3)]]) == 1


def test_pieces_outlast_one_look():
    """the two pieces of the input "priors", each under the priors its pieces case uses: more global sweeps than one look"""
    _, _, cands = T.input_candidates("priors")
    for name in ("prefix", "above_2_33", "high_bits"):
        prior = T.priors_under_test()[name][0]
        first = T.settle(cands[:T.PIECE_CUT], None, prior)[1]
        assert T.jacobi_sweeps(cands[:T.PIECE_CUT], None, prior) > SWEEPS_PER_LOOK
        assert T.jacobi_sweeps(cands[T.PIECE_CUT:], first, prior) > SWEEPS_PER_LOOK
        whole = T.settle(cands, None, prior)
        assert T.settle(cands[T.PIECE_CUT:], first, prior) == (whole[0][T.PIECE_CUT:], whole[1])


def test_cell_cap_input():
    """windows of one tie read would need more than 64 Mi cells with the golden table: the window must grow"""
    t, reads, cands = T.input_candidates("cell_cap")
    out = np.zeros(len(t.cores) + 1, dtype=np.int32)
    import ctypes as C
    ns, nb = C.c_int32(), C.c_int32()
    assert host.lib().scalce_patterns_describe_host(t.blob, len(t.blob), 0, out.ctypes.data, len(out), C.byref(ns), C.byref(nb)) == 0
    nb1 = nb.value + 1
    ntie = len(T.tie_rows(cands))
    assert ntie * nb1 > T.MAX_CELLS and ntie <= 8192 and all(len(c) >= 2 for c in cands)
    assert ntie > T.MAX_CELLS // nb1 == 4301


def test_candidates_and_settle_by_hand():
    cores = ["ACGT", "TTTT", "GG", "ACGTA"]
    assert T.candidates(cores, "CCACGTCC") == [(0, 5)]
    assert T.candidates(cores, "TTTTTACGTCTTTT") == [(1, 3), (0, 8)]      # first appearance, last base of the first occurrence
    assert T.candidates(cores, "GGACGTATTTT") == [(3, 6)]                  # the longest length only
    assert T.candidates(cores, "CCGGC") == [(2, 3)] and T.candidates(cores, "CACAC") == []
    assert T.occurrences(cores, "TTTTT") == [(1, 3), (1, 4)]
    ab, ba = [(0, 3), (1, 7)], [(1, 3), (0, 7)]
    toks, counts = T.settle([ab, ba, ab, [(1, 3)], ab, [], ab])
    #        A=0 B=0 -> A; B=0 A=1 -> A (strictly more); A=2 -> A; fixed B; A=3 B=1 -> A; root; A
    assert toks == [(0, 4), (0, 8), (0, 4), (1, 4), (0, 4), (T.ROOT, 0), (0, 4)] and counts == {0: 5, 1: 1, T.ROOT: 1}
    assert T.settle([ab, ab], prior={1: 1})[0] == [(1, 8), (1, 8)]
    assert T.settle([ab, ab], prior={1: 1, 0: 1})[0] == [(0, 4), (0, 4)]   # equal: the first candidate keeps the read
    assert T.settle([ab], fixed={1: 2}, prior={0: 1 << 33}) == ([(0, 4)], {0: 1, 1: 2})
    assert T.settle([ab], fixed={1: 2}, prior={0: 1}) == ([(1, 8)], {1: 3})
    assert T.cores_of_bin(b"\x05\x00\x01\x00\x00\x00\x1b\x00") == ["AACGT"]
