"""The ingest stage (piece_unpack_t, host_ingest.inc; ingest_tiles2_k, unpack_tiled_k, unpack_k, long_names_k,
kernels_ingest.hpp) on every path and record variant, at the texts where its arithmetic can go wrong.  Every case builds a text
with the builder of tests/ingest_ref.py, runs it through the C ABI (compress, or append for the cases with pieces) and compares,
bit for bit, with the restatement there and with the oracle: q' (SCALCE_OUT_QINPUT), stored name lengths, name cells and names,
tokens and order, every base of every row (SCALCE_OUT_READS decoded back to 2-bit rows in input order), the trigram counters,
mate 2's outputs; Batch.ingest_plan() must be the plan the case is named after, and where the one-pass kernel ran
Batch.quality_plan() must report the tile ranges with exactly the smallest symbol and the span of q'.  No case skips or branches
on the plan it got.  tests/test_ingest_ref_cpu.py has asserted, without a device, that every text is what its case claims.

Which case reaches what (tests/ingest_cases.py; -fastq, -Q, -f, -i, -mate2 behind a name: the record variant)
  ingest_tiles2_k
    the fifteen tails L % 16, both q' store alignments, one or two whole units in front ... lengths: len16 .. len33
    magic division into (record, word) at S = 1, 2, 3 words of stride and W = 1 .. 10 ....... lengths: 60 | 61, 124 | 125, 159, 160
    fused rows and rows back to back ........................................................ lengths: len<L>, len<L>_unfused
    a record that starts on a tile's last two bytes, on the tile, behind it .................. geometry: start16382 .. 16385
    the last newline on the overlap's last byte (taken) and behind it (slow) ................ geometry: tile1_*, tile2_*
    the text ends inside the overlap; its length at every residue mod 16 .................... geometry: text_ends_in_overlap, text_bytes_64k*
    -i: mate 1 inside the tile, mate 2 behind the overlap ................................... geometry: mate1_in_tile_mate2_behind_overlap
    name scan and name cell ................................................................. names: names-*
    every byte on the sequence line, every symbol 0 .. 79, affine and table ................. bytes: all_bytes_*
    tile min / max: the tail unit, an N, the record that crosses ............................ bytes: largest_*, smallest_*
  the fallback (slow, then index_write_k + unpack_tiled_k, fuse_rows_k for fused rows) ....... fallback: long_record_*
  unpack_tiled_k: L = 1 .. 15, 1 .. 257 records, LDS and global side by side, bytewise q' .... tiled: *
  unpack_k: L = 161 .. 300, one and two workgroups ........................................... direct: *
  long_names_k: store offsets across pieces, out[3] per piece ................................ names: long_names_in_two_pieces*
  errors: message, record and length on every path ........................................... errors: *
  consumed, and the remainder fed back ....................................................... test_pieces
"""
import re
import struct

import numpy as np
import pytest

import decode_ref as D
import ingest_cases as IC
import ingest_ref as R
import oraclelib as O
from scalce_amd import host

pytestmark = pytest.mark.gpu
NONE = (500, 500)


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


@pytest.fixture
def ingest_mode(monkeypatch):
    def set_mode(indexed):
        if indexed:
            monkeypatch.setenv("SCALCE_INGEST_INDEXED", "1")
        else:
            monkeypatch.delenv("SCALCE_INGEST_INDEXED", raising=False)
    set_mode(False)
    return set_mode


# ---- the device --------------------------------------------------------------------------------------------------------------
def new_batch(ctx, case, nrec, text_bytes):
    nm = len(case.L)
    b = host.Batch(ctx, case.L[0], max_reads=nrec + 8, max_text=text_bytes + 64, paired=nm == 2, read_len2=case.L[1] if nm == 2 else 0,
                   use_names=case.use_names, no_ac=case.no_ac, qmap=case.qmap, fasta=case.lpr == 2,
                   no_qualities=not case.qout and case.lpr == 4, interleaved=case.il)
    if case.unfuse:
        b.set_fused_rows(False)
    return b


def on_device(texts):
    from gpu_util import device_bytes
    dev = [device_bytes(t) if len(t) else None for t in texts]
    args = []
    for t, d in zip(texts, dev):
        args += [d.data_ptr() if d is not None else None, len(t)]
    return dev, (args + [None, 0])[:4]


def run_whole(ctx, case, e):
    dev, args = on_device(case.texts)
    b = new_batch(ctx, case, e.nrec, max(len(t) for t in case.texts))
    b._keep = dev
    b.compress(*args)
    b.finish()
    return b


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def names_in_input_order(b):
    """SCALCE_OUT_NAMES holds [u8 n][bytes] per record in emission order -> the records in input order"""
    names = b.output(host.OUT_NAMES, 0).tobytes()
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    by_row, pos = [None] * len(perm), 0
    for k in range(len(perm)):
        by_row[int(perm[k])] = names[pos + 1:pos + 1 + names[pos]]
        pos += 1 + names[pos]
    assert pos == len(names), "SCALCE_OUT_NAMES is longer than its records"
    return by_row


def rows_in_input_order(ctx, b, mate, L, perm, n):
    """SCALCE_OUT_READS decoded (decode_ref.unpack_records) and packed again as rows: every base of every row"""
    payload = b.output(host.OUT_READS, mate).tobytes()
    if mate == 0:
        reads, _, ends = D.unpack_records(payload, L, lambda cid: ctx.pattern(cid))
    else:
        reads, ends = D.unpack_records(payload, L, None, has_buckets=False, nrecords=n)[0], None
    assert len(reads) == n
    rows = np.zeros((n, (L + 3) // 4), dtype=np.uint8)
    rows[perm] = R.pack_rows(np.frombuffer(b"".join(reads), dtype=np.uint8).reshape(n, L))
    return rows, ends


def first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return bad[:4]


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert len(got) == len(want), f"{what}: {len(got)} vs {len(want)}"
    assert np.array_equal(got, want), f"{what}: differs first at {first_bad(got, want)} of {len(want)}"


def compare_outputs(ctx, trie, b, case, e):
    """everything the batch holds behind finish() against the restatement `e` and the oracle"""
    n, nm = e.nrec, len(case.L)
    assert b.n_reads == n
    if n == 0:
        return
    # names
    same(b.output(host.OUT_NAMELEN, 0), e.namelen, "stored name lengths")
    cells = b.output(host.OUT_NAMECELLS, 0)
    if case.use_names:
        want = b"".join(bytes([len(x)]) + x[:R.CELL_CHARS].ljust(R.CELL_CHARS, b"\0") for x in e.names)
        same(cells, np.frombuffer(want, dtype=np.uint8), "name cells ([length][15 characters, zero behind the name], 16 bytes per row)")
    else:
        assert len(cells) == 0
    # tokens and order: the oracle's, from the text's own sequence lines
    pat, end = trie.tokenize(e.bases[0])
    operm = trie.order(e.bases[0], pat, end)
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    same(tok[:, 0], pat, "token: core")
    same(tok[:, 1], end, "token: end")
    perm = b.output(host.OUT_PERM, 0, np.uint32).astype(np.int64)
    same(perm, operm, "order")
    if case.use_names:
        got_names = names_in_input_order(b)
        bad = [r for r in range(n) if got_names[r] != e.names[r]]
        assert not bad, f"names differ first at record {bad[:4]}: {got_names[bad[0]]!r} vs {e.names[bad[0]]!r}"
    else:   # (the name stream of a run without names is empty)
        assert len(b.output(host.OUT_NAMES, 0)) == 0 and all(x == b"" for x in e.names)
    for m in range(nm):
        what = f"mate {m + 1}"
        rows, ends = rows_in_input_order(ctx, b, m, case.L[m], perm, n)
        badrow = np.flatnonzero((rows != e.rows[m]).any(axis=1))
        assert len(badrow) == 0, f"{what}: 2-bit rows differ first at records {badrow[:4]}: {rows[badrow[0]]} vs {e.rows[m][badrow[0]]}"
        if ends is not None:
            same(np.asarray(ends)[np.argsort(perm)], end, "the core's end in the records")
        q = b.output(host.OUT_QINPUT, m)
        if not case.qout:
            assert len(q) == 0
            continue
        same(q, e.qp[m], f"{what}: q'")
        if not case.no_ac:
            f4 = O.quality_stream(e.quals[m], e.bases[m], *e.maps[m])[1]
            same(b.output(host.OUT_FREQ4, m, np.uint64) + np.uint64(1), f4, f"{what}: trigram counters")


def check_plans(b, case, plans, piece_qp, front=None):
    """ingest_plan of every mate, and -- where the one-pass kernel wrote q' and the counters ran -- the tile ranges: source 1,
    lo and A exactly the smallest symbol and the span of the piece's q' and the two symbols in front of it"""
    for m, want in enumerate(plans):
        assert b.ingest_plan(m) == want, f"mate {m + 1}: ingest_plan {b.ingest_plan(m)}, predicted {want}"
        if want[0] == R.K_ONE_PASS and case.qout and not case.no_ac:
            lo, A = R.symbol_span(piece_qp[m], NONE if front is None else front[m])
            assert b.quality_plan(m) == (1, lo, A, 1), f"mate {m + 1}: quality_plan {b.quality_plan(m)}, q' spans [{lo}, {lo + A})"


def run_case(ctx, trie, case, ingest_mode):
    ingest_mode(case.indexed)
    e = IC.expect(case)
    assert e.error == case.error and e.plan[-1][:2] == (case.kernel, case.slow)     # (test_ingest_ref_cpu.py holds the rest)
    if case.prefix is not None:
        return run_appended(ctx, trie, case, e)
    if case.error is not None:
        code, rec, aux = case.error
        want = re.escape(f"(ERROR) {R.MESSAGE[code]} [record/block {rec}, aux {aux}]") + "$"
        with pytest.raises(host.ScalceError, match=want):
            run_whole(ctx, case, e)
        return None
    b = run_whole(ctx, case, e)
    check_plans(b, case, e.plan, e.qp)
    compare_outputs(ctx, trie, b, case, e)
    return b


def run_appended(ctx, trie, case, e):
    """the case's text as a second piece behind the rows of `prefix`: plans per piece, consumed, then everything of both"""
    both = [p + t for p, t in zip(case.prefix, case.texts)]
    e0, e_all = IC.expect(case, texts=case.prefix), IC.expect(case, texts=both)
    assert e0.nrec > 0 and e_all.nrec == e0.nrec + e.nrec and e_all.error is None
    b = new_batch(ctx, case, e_all.nrec, max(len(t) for t in both))
    dev0, args0 = on_device(case.prefix)
    used = b.append(*args0, final=False)
    assert list(used[:len(case.prefix)]) == [len(t) for t in case.prefix] == e0.consumed
    check_plans(b, case, e0.plan, e0.qp)
    dev1, args1 = on_device(case.texts)
    used = b.append(*args1, final=True)
    assert list(used[:len(case.texts)]) == [len(t) for t in case.texts] == e.consumed
    front = [tuple(int(x) for x in q.reshape(-1)[-2:]) if q is not None and q.size >= 2 else NONE for q in e0.qp]
    check_plans(b, case, e.plan, e.qp, front)
    b.order(); b.emit(); b.entropy(); b.finish()
    assert b.ingest_plan() == e.plan[0]
    compare_outputs(ctx, trie, b, case, e_all)
    return b


def ids(group):
    return [c.id for c in IC.cases(group)]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(IC.cases("lengths"))), ids=ids("lengths"))
def test_read_lengths(i, ctx, oracle_trie, ingest_mode):
    """L = 16 .. 33, 60 | 61, 124 | 125, 159, 160 through the one-pass kernel -- single-end with fused rows where the batch picks
    them, again with rows back to back, and as mate 2 behind a mate 1 of another length; 15 and 161 on the same inputs take the
    tiled and the direct kernel."""
    case = IC.cases("lengths")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    L = case.L[-1]
    assert b.ingest_plan(len(case.L) - 1)[0] == (1 if 16 <= L <= 160 else 2 if L == 15 else 3)


@pytest.mark.parametrize("i", range(len(IC.cases("geometry"))), ids=ids("geometry"))
def test_tile_geometry(i, ctx, oracle_trie, ingest_mode):
    """One chosen record against the tile and its overlap: see ingest_cases.geometry_cases."""
    run_case(ctx, oracle_trie, IC.cases("geometry")[i], ingest_mode)


@pytest.mark.parametrize("i", range(len(IC.cases("fallback"))), ids=ids("fallback"))
def test_fallback(i, ctx, oracle_trie, ingest_mode):
    """One record that leaves its window -- first, last, across a tile boundary -- in an otherwise ordinary text: `slow`, then the
    indexed kernels over the whole piece (plan [2, 1, 1, ..]); single-end with fused rows, and behind rows the batch holds."""
    case = IC.cases("fallback")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    for m in (range(2) if case.il else [len(case.L) - 1]):
        assert b.ingest_plan(m)[:3] == (2, 1, 1)


@pytest.mark.parametrize("i", range(len(IC.cases("tiled"))), ids=ids("tiled"))
def test_indexed_tiled_kernel(i, ctx, oracle_trie, ingest_mode):
    """unpack_tiled_k by read length (1 .. 15), by the switch, with one workgroup's text beyond its LDS tile, with q' rows that
    start at an odd byte, and under -i with one mate's length outside 16 .. 160."""
    case = IC.cases("tiled")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    assert all(b.ingest_plan(m)[:3] == (2, 0, 1) for m in (range(2) if case.il else [len(case.L) - 1]))


@pytest.mark.parametrize("i", range(len(IC.cases("direct"))), ids=ids("direct"))
def test_direct_kernel(i, ctx, oracle_trie, ingest_mode):
    """unpack_k: L = 161, 255, 256, 300 and 1, 255, 256, 257 records (one workgroup, and two)."""
    case = IC.cases("direct")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    assert b.ingest_plan(len(case.L) - 1)[:3] == (3, 0, 1)


@pytest.mark.parametrize("i", range(len(IC.cases("names"))), ids=ids("names"))
def test_names(i, ctx, oracle_trie, ingest_mode):
    """Stored lengths 0 .. 255, the first space at every phase of the scan, no space in front of a sequence line that begins with
    one, tabs and bytes >= 0x80, a full cell with a comment behind it, the text's first record; names off; long names in two pieces."""
    run_case(ctx, oracle_trie, IC.cases("names")[i], ingest_mode)


@pytest.mark.parametrize("i", range(len(IC.cases("bytes"))), ids=ids("bytes"))
def test_bytes(i, ctx, oracle_trie, ingest_mode):
    """Every byte but the newline at every place of a 16-base unit, every character that maps to 0 .. 79, through the affine
    shortcut and through a lossy table; the largest and the smallest symbol where only one lane sees them."""
    case = IC.cases("bytes")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    if case.span is not None:
        assert b.quality_plan()[1:3] == case.span


@pytest.mark.parametrize("i", range(len(IC.cases("errors"))), ids=ids("errors"))
def test_errors(i, ctx, oracle_trie, ingest_mode):
    """One offending record per text: the message, the record's index and, for a line of the wrong length, the length found,
    exactly; symbol 79 passes, and with -A (no_ac) 80 and a character below the offset pass too."""
    case = IC.cases("errors")[i]
    b = run_case(ctx, oracle_trie, case, ingest_mode)
    assert (b is None) == (case.error is not None)


PIECES = IC.piece_cases()


@pytest.mark.parametrize("i", range(len(PIECES)), ids=[p[0] for p in PIECES])
def test_pieces(i, ctx, oracle_trie, ingest_mode):
    """A piece cut inside a record, behind one, between the mates of a pair, or with one mate ten records ahead: only whole
    records (pairs) both mates hold are taken, `consumed` points behind them, and the remainder in front of the rest of the text
    gives the whole text's outputs."""
    name, whole, cuts, consumed = PIECES[i]
    first = [t[:c] for t, c in zip(whole.texts, cuts)]
    e0, e = IC.expect(whole, texts=first), IC.expect(whole)
    assert e0.consumed == consumed and 0 < e0.nrec < e.nrec
    b = new_batch(ctx, whole, e.nrec, max(len(t) for t in whole.texts))
    dev0, args0 = on_device(first)
    used = b.append(*args0, final=False)
    assert list(used[:len(first)]) == consumed, f"{name}: consumed {used}, the restatement says {consumed}"
    assert b.n_reads == e0.nrec
    check_plans(b, whole, e0.plan, e0.qp)
    rest = [t[u:] for t, u in zip(whole.texts, consumed)]
    e1 = IC.expect(whole, texts=rest)
    dev1, args1 = on_device(rest)
    used = b.append(*args1, final=True)
    assert list(used[:len(rest)]) == [len(t) for t in rest]
    front = [tuple(int(x) for x in q.reshape(-1)[-2:]) for q in e0.qp]
    check_plans(b, whole, e1.plan, e1.qp, front)
    b.order(); b.emit(); b.entropy(); b.finish()
    compare_outputs(ctx, oracle_trie, b, whole, e)


@pytest.mark.parametrize("variant", IC.VARIANTS)
def test_nothing_ingested(variant, ctx, oracle_trie, ingest_mode):
    """out[0] = 0: a new batch, and a piece that holds no whole record (pair); the next piece reports its own plan."""
    lay = IC.Layout(variant, 50, 40, 73)
    case = lay.case("nothing")
    e = IC.expect(case)
    b = new_batch(ctx, case, e.nrec, max(len(t) for t in case.texts))
    nm = len(case.L)
    assert all(b.ingest_plan(m) == (0, 0, 0, 0) for m in range(nm))
    stub = [t[:30] for t in case.texts]
    assert IC.expect(case, texts=stub).nrec == 0
    dev0, args0 = on_device(stub)
    used = b.append(*args0, final=False)
    assert tuple(used) == (0, 0) and b.n_reads == 0
    assert all(b.ingest_plan(m) == (0, 0, 0, 0) for m in range(nm))
    dev1, args1 = on_device(case.texts)
    b.append(*args1, final=True)
    check_plans(b, case, e.plan, e.qp)
    assert all(b.ingest_plan(m)[0] == 1 for m in range(nm))
    b.order(); b.emit(); b.entropy(); b.finish()
    compare_outputs(ctx, oracle_trie, b, case, e)
    b.reset()
    assert all(b.ingest_plan(m) == (0, 0, 0, 0) for m in range(nm))
