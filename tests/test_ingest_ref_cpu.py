"""No device: the restatement of the ingest stage (tests/ingest_ref.py) against what exists already -- the oracle's pack_read,
the golden vectors of the reference's own objects -- and every crafted text of tests/ingest_cases.py against what its case claims
to be: where the chosen record starts and ends, what the text's length is, which plan the restatement predicts."""
import hashlib
import os

import numpy as np
import pytest

import ingest_cases as IC
import ingest_ref as R
import oraclelib as O
from scalce_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the 2-bit rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 15, 16, 17, 19, 100, 161, 1000, 2498])
def test_rows_are_pack_read(L):
    rng = np.random.default_rng(L)
    bases = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, size=(40, L))]
    rows = R.pack_rows(bases)
    assert rows.shape == (40, (L + 3) // 4)
    for r in range(40):
        assert np.array_equal(rows[r], O.pack_read(bases[r], 0, 0)), r


def test_rows_of_every_byte():
    """all 255 byte values a sequence line can hold, at each of the four places of a packed byte"""
    for place in range(4):
        for v in range(256):
            if v == 10:
                continue
            row = np.frombuffer(b"TTTT", dtype=np.uint8).copy()
            row[place] = v
            want = O.pack_read(row, 0, 0)
            assert np.array_equal(R.pack_rows(row[None, :])[0], want), (place, v)
            code = {67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(v, 0)     # getval, const.cpp:47-49
            assert (int(want[0]) >> (6 - 2 * place)) & 3 == code, (place, v)


# ---- the golden vectors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se100", "se150_text", "se36_ties"])
def test_restatement_matches_golden_vectors(name, patterns_blob):
    """q', names and the packed records of the reference's own objects: the restatement's rows, rotated around the core the
    golden tokens name and packed again, are the bytes the reference wrote."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    kw = eval(str(g["kw"]))  # noqa: S307 - literal dict written by make_golden.py
    n, L = int(g["n"]), int(g["L"])
    bases, quals = synth.reads_and_quals(n, L, seed=int(g["seed"]), **kw)
    text = synth.fastq_bytes(bases, quals)
    out = R.ingest(text, L)
    assert out.nrec == n and out.error is None and out.consumed == len(text)
    assert np.array_equal(out.bases[0], bases) and np.array_equal(out.quals[0], quals)
    assert sha(out.qp[0]) == str(g["sha_qual"])
    assert sha(R.trigram_counts(out, 0)) == str(g["sha_freq4"])
    names = b"".join(bytes([len(x)]) + x for x in out.names)
    assert sha(np.frombuffer(names, dtype=np.uint8)) == str(g["sha_names"])
    trie = O.Trie(text=str(g["ptxt"]).encode()) if "ptxt" in g else O.Trie(blob=patterns_blob)
    lens = trie.pattern_lens()
    packed = []
    for r in range(n):
        codes = np.zeros(4 * out.rows[0].shape[1], dtype=np.uint8)
        for k in range(4):
            codes[k::4] = (out.rows[0][r] >> (6 - 2 * k)) & 3
        codes = codes[:L]
        pat, end = int(g["tok"][r, 0]), int(g["tok"][r, 1])
        lvl = int(lens[pat]) if pat >= 0 and end else 0
        rot = np.concatenate([codes[end:], codes[:end - lvl]]) if end else codes      # output_read: behind the core, then in front
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rot]
        packed.append(R.pack_rows(letters[None, :])[0] if len(letters) else np.zeros(0, dtype=np.uint8))
    assert sha(np.concatenate(packed)) == str(g["sha_packed"])
    assert np.array_equal(np.concatenate(packed), g["packed"])


# ---- names, q', errors, consumed on small texts written out by hand -------------------------------------------------------
def test_names_and_consumed_by_hand():
    text = b"@a b c\nACGT\n+x\nIIII\n@\nacgn\n+\n!!!!\n@ only comment\nNNNN\n+\nJJJJ\n@tail"
    out = R.ingest(text, 4)
    assert out.nrec == 3 and out.names == [b"a", b"", b""] and out.consumed == len(text) - 5 and out.error is None
    assert out.rows[0].tolist() == [[0b00011011], [0b00011000], [0]]
    assert out.qp[0].tolist() == [[40] * 4, [0] * 4, [0] * 4]          # 'n' is not 'N': its '!' is symbol 0 anyway
    assert R.ingest(text, 4, take=2).consumed == text.index(b"@ only")
    assert R.ingest(b"@r\nAn\n+\nI5\n", 2).qp[0].tolist() == [[40, 20]]        # 'n' keeps its symbol
    assert R.ingest(b"@r\nAN\n+\nI5\n", 2).qp[0].tolist() == [[40, 0]]         # 'N' forces 0
    assert R.ingest(b">r 1\nACGT\n>s\nTTTT\n", 4, lpr=2).names == [b"r", b"s"]
    il = R.ingest(b"@p/1\nAC\n+\nII\n@p/2\nGTT\n+\nIII\n", (2, 3), interleave=True)
    assert il.nrec == 1 and il.names == [b"p/1"] and il.rows[1].tolist() == [[0b10111100]]


def test_errors_by_hand():
    ok = b"@r\nACGT\n+\nIIII\n"
    assert R.ingest(ok + b"@s\nACG\n+\nIIII\n", 4).error == (R.E_READLEN, 1, 3)
    assert R.ingest(ok + b"@s\nACGTA\n+\nIIII\n", 4).error == (R.E_READLEN, 1, 5)
    assert R.ingest(ok + b"@s\nACGT\n+\nIII\n", 4).error == (R.E_READLEN, 1, 4)
    assert R.ingest(ok + b"\nACGT\n+\nIIII\n", 4).error == (R.E_NAMELEN, 1, 0)
    assert R.ingest(ok + b"@" + b"n" * 256 + b"\nACGT\n+\nIIII\n", 4).error == (R.E_NAMELEN, 1, 0)
    assert R.ingest(ok + b"@" + b"n" * 255 + b" c\nACGT\n+\nIIII\n", 4).error is None
    q80 = ok + b"@s\nACGT\n+\nIII" + bytes([33 + 80]) + b"\n"
    assert R.ingest(q80, 4).error == (R.E_SYMBOL, 1, 0) and R.ingest(q80, 4, no_ac=True).error is None
    assert R.ingest(ok + b"@s\nACGT\n+\nIII" + bytes([33 + 79]) + b"\n", 4).error is None
    below = R.ingest(ok + b"@s\nACGT\n+\nIII \n", 4)
    assert below.error == (R.E_SYMBOL, 1, 0) and below.qp[0][1, 3] == 255
    assert R.ingest(ok + b"@s\nACGN\n+\nIII" + bytes([33 + 80]) + b"\n", 4).error is None      # under an N: symbol 0


def test_plan_rule_by_hand():
    """the fallback rule on texts of two records: one that ends on the last byte of its window, one that ends behind it"""
    def two(extra):
        a = R.Rec(b"a", b"A" * 20, b"I" * 20)
        b = R.Rec(b"b", b"C" * 20, b"I" * 20)
        c = R.Rec(b"c", b"G" * 20, b"I" * 20)
        recs = [a, b, c]
        R.start_at(recs, 1, 100)
        R.end_at(recs, 1, IC.W - 1 + extra)
        return R.join(recs)
    assert R.ingest(two(0), 20).plan == [(R.K_ONE_PASS, 0, 0, 0)]
    assert R.ingest(two(1), 20).plan == [(R.K_TILED, 1, 1, 0)]
    assert R.ingest(two(1), 20, take=1).plan == [(R.K_ONE_PASS, 0, 0, 0)]        # the long record is not taken
    assert R.ingest(two(0), 20, indexed=True).plan == [(R.K_TILED, 0, 1, 0)]
    assert R.ingest(b"", 20).plan == [(R.K_NONE, 0, 0, 0)]
    named = R.join([R.Rec(b"n" * 16 + b" c", b"A" * 20, b"I" * 20), R.Rec(b"m" * 15, b"A" * 20, b"I" * 20)])
    assert R.ingest(named, 20).plan == [(R.K_ONE_PASS, 0, 1, 16)]
    assert R.ingest(named, 20, use_names=False).plan == [(R.K_ONE_PASS, 0, 0, 0)]
    assert R.ingest(R.join([R.Rec(b"r", b"A" * 161, b"I" * 161)]), 161).plan == [(R.K_DIRECT, 0, 1, 0)]
    # more than ING_NLMAX newlines in a window: out of reach for a text whose lines have their lengths -- a name line is at least
    # one byte and its newline, a sequence line at least 16 bases and its newline, in every variant
    assert (IC.W * 2) // (2 + 17) < R.ING_NLMAX
    assert R.ONE_PASS_L == (16, 160) and R.UNP_RPB * 160 <= R.UNP_Q_CAP < R.UNP_RPB * 161


# ---- the crafted texts are what they claim to be ------------------------------------------------------------------------------
def record_span(text, lpr, k):
    """(first byte, last newline) of the k-th record of lpr lines"""
    nl = R.lines_of(text)
    return (int(nl[lpr * k - 1]) + 1 if k else 0), int(nl[lpr * k + lpr - 1])


def check_claims(case):
    e = IC.expect(case)
    assert len(case.texts[-1]) <= 200 * 1024 and e.nrec <= 1000, "a case stays small"
    assert e.error == case.error, f"{case.id}: the restatement finds {e.error}"
    assert e.plan[-1][:2] == (case.kernel, case.slow), f"{case.id}: the restatement predicts {e.plan}"
    if case.slow:
        assert all(p[:3] == (p[0], 1, 1) and p[0] in (R.K_TILED, R.K_DIRECT) for p in (e.plan if case.il else e.plan[-1:]))
    for t, k, start, end in case.claims:
        s, z = record_span(case.texts[t], case.lpr, k)
        assert start is None or s == start, f"{case.id}: record {k} starts at {s}, not {start}"
        assert end is None or z == end, f"{case.id}: record {k} ends at {z}, not {end}"
    if case.name_line_ends_behind is not None:
        t, k, start, _ = case.claims[0]
        assert int(R.lines_of(case.texts[t])[case.lpr * k]) >= case.name_line_ends_behind > start
    if case.text_bytes is not None:
        assert len(case.texts[-1]) == case.text_bytes and case.texts[-1].endswith(b"\n")
    if case.span is not None:
        assert R.symbol_span(e.qp[-1]) == case.span
    if case.wg_in_lds is not None:
        nl = R.lines_of(case.texts[0])
        for wg, fits in case.wg_in_lds.items():   # unpack_tiled_k: span0 rounded down to 16 .. span1
            r0, r1 = wg * R.UNP_RPB, min((wg + 1) * R.UNP_RPB, e.nrec)
            span0 = int(nl[case.lpr * r0 - 1]) + 1 if r0 else 0
            span1 = int(nl[case.lpr * r1 - 1]) + 1
            assert (span1 - (span0 & ~15) <= R.unp_text_cap(case.L[0])) == fits, (wg, span1 - span0)
    return e


@pytest.mark.parametrize("group", sorted(IC.GROUPS))
def test_crafted_texts_are_what_they_claim(group):
    got = [check_claims(c) for c in IC.cases(group)]
    assert len(got) > 0


def test_geometry_windows():
    """the geometry cases, window by window: the chosen record's newline against the end of the window it starts in, and the
    newlines that window holds"""
    for case in IC.cases("geometry"):
        text = case.texts[0]
        nl = R.lines_of(text)
        RL = case.lpr * (2 if case.il else 1)
        for t, k, start, end in case.claims:
            if start is None or end is None:
                continue
            unit = k // 2 if case.il else k
            ustart, uend = (int(nl[RL * unit - 1]) + 1 if unit else 0), int(nl[RL * unit + RL - 1])
            a, z = R.windows(len(text))[ustart // R.ING_TILE]
            held = int(np.searchsorted(nl, z) - np.searchsorted(nl, a))
            assert held <= R.ING_NLMAX
            assert (uend >= z) == bool(case.slow), f"{case.id}: the pair / record ends at {uend}, its window at {z}"
            if "last_overlap_byte" in case.id:
                assert uend == z - 1 and ustart // R.ING_TILE == (start // R.ING_TILE)
            if "behind_overlap" in case.id and "mate1" not in case.id:
                assert uend == z


def test_every_plan_is_reached_in_every_variant():
    """each kernel, and both values of `slow`, for FASTQ, -Q, -f, -i and mate 2"""
    seen = {}
    for group in IC.GROUPS:
        for c in IC.cases(group):
            if c.error is None:
                seen.setdefault(c.id.rsplit("-", 1)[1], set()).add((c.kernel, c.slow))
    for v in IC.VARIANTS:
        assert {(1, 0), (2, 0), (3, 0), (2, 1)} <= seen[v], (v, seen[v])


def test_pieces_are_cut_where_they_claim():
    for name, whole, cuts, consumed in IC.piece_cases():
        first = [t[:c] for t, c in zip(whole.texts, cuts)]
        e = IC.expect(whole, texts=first)
        assert e.consumed == consumed, (name, e.consumed, consumed)
        assert e.error is None and IC.expect(whole).error is None
        if name == "cut_mid_line":
            assert not first[0].endswith(b"\n")
        if name == "cut_behind_a_record":
            assert e.consumed[0] == len(first[0])
        if name == "mate1_ten_records_ahead":
            assert R.ingest(first[0], whole.L[0]).nrec == e.nrec + 10
