"""The quality statistics stage (scalce_batch_quality, host_ingest.inc; tile_minmax_reduce_k, sym_range_k, tri_prev_k,
tri_range_k, trigram_pass_k, tri_check_k, kernels_ingest.hpp) driven alone -- ingest or append, quality, finish -- at the
inputs where its counting paths change.  Every one of the 512000 counters (SCALCE_OUT_FREQ4) and every q' byte
(SCALCE_OUT_QINPUT) is compared with the oracle (oraclelib.quality_stream), which is first compared with a numpy
restatement of the same count (trigram_table below; test_quality_oracle_cpu.py does that without a device).  Every case
asserts on the CPU that its input is what it claims to be, and Batch.quality_plan() that the host took the path meant.

The oracle's table starts at 1 in every cell at a mate's very first symbol (qualities.cpp:191-196) and at 0 when symbols are
carried in; the device keeps raw counts, so `device + 1 == oracle` exactly when prev[1] is 500.

Which case reaches which path:
  passes of trigram_pass_k, width = 61000 // A^2 leading symbols each
    one pass, the `fast` loop (A <= 39) ................ test_alphabet_spans_* A = 1, 2, 39; test_guard_bit constant
    boundary 39 | 40 between the fast and the tested loop  test_alphabet_spans_* A = 39, 40 (lo = 0 and lo = 80 - A)
    two passes .......................................... A = 40, 41
    the third launch, passes [2, 20) in one kernel ...... A = 55 (3 passes), 79, 80 (9 passes)
    a last pass with fewer than `width` leading symbols . A = 40 (38 + 2), 41 (36 + 5), 55 (20 + 20 + 15), 79 (8 x 9 + 7), 80 (8 x 9 + 8)
    an odd `used`: one live 16-bit field in the last word  A = 1, 39 (59319), 41 pass 1 (5 x 1681), 55 pass 2 (15 x 3025), 79 pass 8
  the guard bit (a field reaches 0x8000) ................ test_guard_bit: fast loop (constant), tested loop (ends_0_79,
                                                          whole_alphabet), both again with 64 workgroups (front)
  where the range comes from
    tile ranges of ingest_tiles2_k (source 1) ........... every case with 16 <= L <= 160 and the one-pass ingest
    sym_range_k (source 2), its scalar tail ............. test_flat_rows_and_sym_range (n % 16 = 0, 1, 15, n < 16), paired indexed
    the whole alphabet (source 3), 80 symbols present ... test_alphabet_spans_single indexed, test_guard_bit whole_alphabet
  row geometry under fused rows
    a unit put together from two rows (L % 16 != 0) ..... test_fused_row_geometry L = 20, 36, 100
    adv_r / adv_c (1024 symbols on) ..................... every L there: 1024 % L = 0, 4, 16, 24, 16, 64
    the piece's last unit is short ...................... L = 20 (NP = 1, 3277), 36, 100 (n % 16 != 0)
    one tile, one tile + one unit, one tile + 4 symbols . L = 16 x 4096, 16 x 4097, 20 x 3277
  the flat path's 16-byte loads at any residue mod 16 ... test_pieces_flat_L75
  what lies in front of a piece (tri_prev_k)
    symbols_before >= 2, 1, 0 ........................... test_pieces_one_record_each (L = 1, 2), every pieces test
    qprev of the C ABI and tri_expected ................. test_qprev_*
    the range covers the symbols in front ............... test_piece_widens_the_alphabet, test_piece_narrower_than_what_it_follows
  the side stream with 64 workgroups (quality_beside) ... test_guard_bit via front
  nothing behind the stage assumes 41 symbols ........... test_full_alphabet_end_to_end
"""
import functools

import numpy as np
import pytest

import oraclelib as O
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
IDENT = np.arange(128)
TILE = 65536           # TRI_TILE: symbols a wave takes at a time
FIELDS = 61000         # 2 * TRI_CAP: 16-bit counters in LDS
NONE = (500, 500)


# ---- the reference ---------------------------------------------------------------------------------------------------

def trigram_table(qp, prev=NONE):
    """The oracle's table restated: one count per symbol of the flat stream whose two predecessors exist (prev = the two in
    front of the stream, 500 = none), and one more in every cell when the stream begins the mate (prev[1] = 500)."""
    flat = np.concatenate([np.asarray(prev, dtype=np.int64), np.asarray(qp, dtype=np.int64).reshape(-1)])
    a, b, c = flat[:-2], flat[1:-1], flat[2:]
    have = (a < 256) & (b < 256)
    t = np.bincount(((a * 80 + b) * 80 + c)[have], minlength=512000).astype(np.uint64)
    return t + np.uint64(1 if prev[1] >= 256 and len(c) else 0)


def reference(sym, bases, prev=NONE):
    """(q', table) of the oracle for symbols `sym` (N, L) written as characters 33 + symbol; the restatement must agree."""
    qp, f4 = O.quality_stream((sym + 33).astype(np.uint8), bases, 33, IDENT, prev=prev)
    mine = trigram_table(qp, prev)
    assert np.array_equal(f4, mine), f"oracle and restatement differ at {np.flatnonzero(f4 != mine)[:5]}"
    return qp, f4


def layout(A):
    """trigram_pass_k's passes for a span of A symbols: the 16-bit fields each pass uses (`used`), width = 61000 // A^2
    leading symbols of A^2 fields per pass, fewer in the last."""
    width = FIELDS // (A * A)
    return [min(width, A - d0) * A * A for d0 in range(0, A, width)]


def passes(A):
    return len(layout(A))


def span(*parts):
    """(lo, A) of the symbols below 80 in the parts."""
    s = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
    s = s[s < 80]
    return int(s.min()), int(s.max() - s.min() + 1)


def hot_in_first_tile(qp, tri, prev=NONE):
    """How often trigram `tri` ends inside the first 65536 symbols of the stream: what one wave adds to one field."""
    flat = np.concatenate([np.asarray(prev, dtype=np.int64), np.asarray(qp, dtype=np.int64).reshape(-1)[:TILE]])
    return int(((flat[:-2] == tri[0]) & (flat[1:-1] == tri[1]) & (flat[2:] == tri[2])).sum())


def source_rule(L, single_end, indexed):
    """scalce_batch_quality's branch for short names: 1 = tile ranges (the one-pass ingest ran), 3 = the whole alphabet (fused
    rows without tile ranges), 2 = sym_range_k."""
    if 16 <= L <= 160 and not indexed:
        return 1
    return 3 if single_end and L % 4 == 0 and 16 <= L <= 160 else 2


def want_plan(source, piece, front=NONE):
    """quality_plan() of a piece with symbols `piece` behind the two symbols `front`."""
    if source == 3:
        return (3, 0, 80, 1)
    lo, A = span(piece, front)
    return (source, lo, A, 1)


# ---- the device ------------------------------------------------------------------------------------------------------

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


@functools.lru_cache(maxsize=None)
def random_bases(n, L, seed=1):
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng([seed, n, L]).integers(0, 4, size=(n, L))]
    b.setflags(write=False)
    return b


def fastq(sym, bases, suffix=""):
    return synth.fastq_bytes_fast(bases, (sym + 33).astype(np.uint8), prefix="", suffix=suffix)


def new_batch(ctx, syms, nrec, text_bytes, qprev=None):
    L = [s.shape[1] for s in syms]
    return host.Batch(ctx, L[0], max_reads=nrec + 8, max_text=text_bytes + 64, paired=len(syms) == 2,
                      read_len2=L[1] if len(syms) == 2 else 0, qprev=qprev)


def run_stage(ctx, syms, bases, qprev=None, via="ingest"):
    """The stage alone over one piece per mate: ingest, quality, finish (via = "front": scalce_batch_front, which puts the
    stage on the side stream beside the tie-break)."""
    from gpu_util import device_bytes
    texts = [fastq(s, b, suffix="/%d" % (m + 1) if len(syms) == 2 else "") for m, (s, b) in enumerate(zip(syms, bases))]
    dev = [device_bytes(t) for t in texts]
    b = new_batch(ctx, syms, len(syms[0]), max(len(t) for t in texts), qprev)
    if via == "front":
        b.front(dev[0].data_ptr(), len(texts[0]), dev[1].data_ptr() if len(dev) == 2 else None, len(texts[1]) if len(dev) == 2 else 0)
    else:
        for m, t in enumerate(texts):
            b.ingest(m, dev[m].data_ptr(), len(t))
        b.quality()
    b.finish()   # a total that tri_check_k finds wrong surfaces here
    b._keep = dev
    return b


def same_table(b, mate, f4, prev=NONE, what=""):
    dev = b.output(host.OUT_FREQ4, mate, np.uint64)
    got = dev + np.uint64(1 if prev[1] >= 256 else 0)
    bad = np.flatnonzero(got != f4)
    cells = [(int(i) // 6400, int(i) // 80 % 80, int(i) % 80, int(got[i]), int(f4[i])) for i in bad[:4]]
    assert len(bad) == 0, f"{what} mate {mate + 1}: {len(bad)} counters differ; (a, b, c, device, oracle) = {cells}"


def same_symbols(b, mate, qp, what=""):
    q = b.output(host.OUT_QINPUT, mate)
    want = qp.reshape(-1)
    assert len(q) == len(want), f"{what} mate {mate + 1}: {len(q)} vs {len(want)} q' bytes"
    bad = np.flatnonzero(q != want)
    assert len(bad) == 0, f"{what} mate {mate + 1}: q' differs first at {bad[:4]}"


def check_one_piece(ctx, syms, bases, sources, qprev=None, via="ingest", what=""):
    """One piece per mate: table, q' and plan of every mate.  Returns the batch."""
    prevs = [NONE, NONE] if qprev is None else [tuple(qprev[0]), tuple(qprev[1])]
    refs = [reference(s, bs, prevs[m]) for m, (s, bs) in enumerate(zip(syms, bases))]
    b = run_stage(ctx, syms, bases, qprev=qprev, via=via)
    for m, (qp, f4) in enumerate(refs):
        assert b.quality_plan(m) == want_plan(sources[m], qp, prevs[m]), f"{what} mate {m + 1}: plan"
        same_table(b, m, f4, prevs[m], what)
        same_symbols(b, m, qp, what)
    return b


# ---- a. alphabet spans and pass counts ---------------------------------------------------------------------------------

SPANS = [(0, 1), (0, 2), (0, 39), (0, 40), (0, 41), (0, 55), (0, 79), (0, 80), (79, 1), (41, 39), (40, 40)]
PASSES = {1: 1, 2: 1, 39: 1, 40: 2, 41: 2, 55: 3, 79: 9, 80: 9}


@functools.lru_cache(maxsize=None)
def uniform_case(lo, A, n, L):
    sym = (lo + np.random.default_rng([lo, A, n, L]).integers(0, A, size=(n, L))).astype(np.uint8)
    bases = random_bases(n, L)
    qp, _ = reference(sym, bases)
    assert span(qp) == (lo, A) and passes(A) == PASSES[A], "the case is not what it claims to be"
    return sym, bases


@pytest.mark.parametrize("indexed", [False, True], ids=["one_pass", "indexed"])
@pytest.mark.parametrize("lo,A", SPANS)
def test_alphabet_spans_single(lo, A, indexed, ctx, ingest_mode):
    """1000 x 100 single-end (fused rows), symbols uniform over [lo, lo + A): tile ranges -> the span itself, `inside` set;
    under the indexed ingest the whole alphabet is laid out whatever the data (nine passes, no fast loop)."""
    ingest_mode(indexed)
    sym, bases = uniform_case(lo, A, 1000, 100)
    b = check_one_piece(ctx, [sym], [bases], [source_rule(100, True, indexed)], what=f"[{lo}, {lo + A})")
    plan = b.quality_plan()
    assert plan[3] == 1 and plan[:3] == ((3, 0, 80) if indexed else (1, lo, A))


@pytest.mark.parametrize("indexed", [False, True], ids=["one_pass", "indexed"])
@pytest.mark.parametrize("i", range(len(SPANS)))
def test_alphabet_spans_paired(i, indexed, ctx, ingest_mode):
    """The same spans with rows that lie flat: a paired batch, 100 and 75 symbols, another span per mate -- the plan is the
    mate's own.  Tile ranges, or sym_range_k under the indexed ingest."""
    ingest_mode(indexed)
    (lo1, A1), (lo2, A2) = SPANS[i], SPANS[(i + 3) % len(SPANS)]
    s1, b1 = uniform_case(lo1, A1, 1000, 100)
    s2, b2 = uniform_case(lo2, A2, 1000, 75)
    src = source_rule(100, False, indexed)
    assert src == source_rule(75, False, indexed) == (2 if indexed else 1)
    b = check_one_piece(ctx, [s1, s2], [b1, b2], [src, src], what=f"[{lo1}, {lo1 + A1}) | [{lo2}, {lo2 + A2})")
    assert b.quality_plan(0) == (src, lo1, A1, 1) and b.quality_plan(1) == (src, lo2, A2, 1)
    assert b.quality_plan(0) != b.quality_plan(1)


# ---- b. the guard bit --------------------------------------------------------------------------------------------------

S_HOT = 40


@functools.lru_cache(maxsize=None)
def guard_case(variant):
    """-> (symbols, bases, {trigram: hits inside the first tile})"""
    if variant == "period3":   # s, s, s + 1 along the flat stream
        sym = (S_HOT + (np.arange(1400 * 100) % 3 == 2)).astype(np.uint8).reshape(1400, 100)
    else:
        sym = np.full((700, 100), S_HOT, dtype=np.uint8)
        if variant == "ends_0_79":
            sym.flat[0], sym.flat[-1] = 0, 79
    bases = random_bases(len(sym), 100)
    qp, f4 = reference(sym, bases)
    s = S_HOT
    tris = [(s, s, s + 1), (s, s + 1, s), (s + 1, s, s)] if variant == "period3" else [(s, s, s)]
    return sym, bases, qp, f4, {t: hot_in_first_tile(qp, t) for t in tris}


@pytest.mark.parametrize("variant,via", [("constant", "ingest"), ("ends_0_79", "ingest"), ("period3", "ingest"),
                                         ("whole_alphabet", "ingest"), ("constant", "front"), ("ends_0_79", "front")])
def test_guard_bit(variant, via, ctx, ingest_mode):
    """One trigram hit more than 32768 times by ONE wave (a 64 KiB tile of one symbol): the field reaches 0x8000, is taken
    down and 32768 go to the global table -- in the fast loop (constant: A = 1), in the tested loop (the same stream between a
    0 and a 79: A = 80, s = 40 counted in pass 4; whole_alphabet: the constant stream under the indexed ingest, all 80 symbols
    laid out for one).  period3 (s, s, s + 1): three fields of 46666 hits whose 21845 per tile pass 0x8000 when one
    workgroup's waves take more than one of the three tiles, and leave remainders that differ.  front: the same through
    scalce_batch_front, where the stage runs beside the tie-break with 64 workgroups."""
    ingest_mode(variant == "whole_alphabet")
    sym, bases, qp, f4, hot = guard_case("constant" if variant == "whole_alphabet" else variant)
    lo, A = span(qp)
    s = S_HOT
    if variant == "period3":
        assert (lo, A) == (s, 2) and all(v in (21844, 21845) for v in hot.values())
        assert all(int(f4[(t[0] * 80 + t[1]) * 80 + t[2]]) - 1 in (46666, 46667) for t in hot)   # past 32768 over three tiles
    elif variant == "ends_0_79":
        assert (lo, A) == (0, 80) and passes(A) == 9 and (s - lo) // (FIELDS // (A * A)) == 4 and hot[(s, s, s)] == 65533
    else:
        assert (lo, A) == (s, 1) and passes(A) == 1 and hot[(s, s, s)] == 65534
    assert variant == "period3" or hot[(s, s, s)] >= 32768
    src = source_rule(100, True, variant == "whole_alphabet")
    b = run_stage(ctx, [sym], [bases], via=via)
    assert b.quality_plan() == want_plan(src, qp), f"{variant}: plan"
    if variant == "whole_alphabet":
        assert b.quality_plan() == (3, 0, 80, 1)
    if via == "front":   # the tokenizer got as far as its window sweeps: that is where the stage is forked to the side stream
        assert b.stats()["tie_reads"] > 0
    same_table(b, 0, f4, what=variant)
    same_symbols(b, 0, qp, what=variant)


# ---- c. row geometry under fused rows -----------------------------------------------------------------------------------

GEOMETRY = [(16, 4096), (16, 4097), (16, 1), (20, 3277), (20, 1), (36, 3000), (100, 2000), (144, 1300), (160, 1200)]


@pytest.mark.parametrize("A", [39, 80])
@pytest.mark.parametrize("L,NP", GEOMETRY)
def test_fused_row_geometry(L, NP, A, ctx, ingest_mode):
    """Fused rows (single-end, L % 4 == 0, 16 .. 160: qstride != L).  n = NP L is one tile exactly (16 x 4096), one tile and
    one unit (16 x 4097), one tile and four symbols (20 x 3277), one unit (16 x 1), one unit and four symbols (20 x 1), and a
    few thousand rows.  The symbol is a function of (row, column): a unit read from the wrong row lands in other cells."""
    assert L % 4 == 0 and 16 <= L <= 160 and NP * L <= 200000
    n = NP * L
    claims = {(16, 4096): n == TILE, (16, 4097): n == TILE + 16, (20, 3277): n == TILE + 4, (16, 1): n == 16, (20, 1): n == 20}
    assert claims.get((L, NP), n > TILE)
    r, c = np.arange(NP)[:, None], np.arange(L)[None, :]
    sym = ((7 * r + 3 * c) % A).astype(np.uint8)
    bases = random_bases(NP, L)
    qp, _ = reference(sym, bases)
    if NP >= A:
        assert span(qp) == (0, A) and passes(A) == (1 if A == 39 else 9)
    check_one_piece(ctx, [sym], [bases], [1], what=f"{NP} x {L}, A = {A}")


# ---- d. flat rows and sym_range_k ----------------------------------------------------------------------------------------

def flat_shapes():
    """(L, NP): for every L record counts that leave n % 16 at 0, 1 and 15 where L allows it, and one with n < 16."""
    out = []
    for L in (1, 2, 3, 8, 15, 75, 161, 200):
        first = max(2, 3000 // L)
        for r in (0, 1, 15):
            np_ = next((k for k in range(first, first + 16) if k * L % 16 == r), None)
            if np_ is not None:
                out.append((L, np_))
        if L < 16:
            out.append((L, max(1, 15 // L)))
    return out


FLAT = [(L, NP, False) for L, NP in flat_shapes()] + [(75, NP, True) for L, NP in flat_shapes() if L == 75]


@pytest.mark.parametrize("where", ["largest_last", "smallest_first"])
@pytest.mark.parametrize("L,NP,indexed", FLAT)
def test_flat_rows_and_sym_range(L, NP, indexed, where, ctx, ingest_mode):
    """Rows that lie flat, single-end: sym_range_k (L outside 16 .. 160, or 75 under the indexed ingest; tile ranges at 75
    otherwise) with n % 16 = 0, 1, 15 and n < 16.  The largest symbol occurs once, as the very last -- in the scalar tail when
    there is one -- or the smallest once, as the very first: a range that misses either loses the trigrams around it."""
    ingest_mode(indexed)
    n = NP * L
    sym = (10 + np.random.default_rng([L, NP]).integers(0, 40, size=n)).astype(np.uint8)
    if where == "largest_last":
        sym[-1] = 70
    else:
        sym[0] = 3
    sym = sym.reshape(NP, L)
    bases = random_bases(NP, L)
    qp, _ = reference(sym, bases)
    lo, A = span(qp)
    assert (lo + A - 1 == 70 and (qp == 70).sum() == 1) if where == "largest_last" else (lo == 3 and (qp == 3).sum() == 1)
    src = source_rule(L, True, indexed)
    assert src == (1 if L == 75 and not indexed else 2)
    check_one_piece(ctx, [sym], [bases], [src], what=f"{NP} x {L}, n % 16 = {n % 16}")


# ---- e. pieces -----------------------------------------------------------------------------------------------------------

def run_pieces(ctx, sym, bases, sizes, source, qprev=None, what=""):
    """The records appended in pieces of whole records (no tokenization): after every piece the table is the oracle's of the
    records so far and the plan that of the piece behind the two symbols in front of it; at the end every q' byte."""
    from gpu_util import device_bytes
    N, L = sym.shape
    assert sum(sizes) == N
    prev = NONE if qprev is None else tuple(qprev[0])
    b = new_batch(ctx, [sym], N, len(fastq(sym, bases)), qprev)
    flat = np.concatenate([np.asarray(prev, dtype=np.int64), sym.reshape(-1).astype(np.int64)])  # (no N bases: q' is the symbol)
    at, keep = 0, []
    for k, sz in enumerate(sizes):
        piece = fastq(sym[at:at + sz], bases[at:at + sz])
        d = device_bytes(piece)
        keep.append(d)
        used = b.append(d.data_ptr(), len(piece), final=k == len(sizes) - 1, flags=host.APPEND_NO_TOKENIZE)
        b.finish()
        assert used[0] == len(piece) and b.n_reads == at + sz
        front = tuple(int(x) for x in flat[at * L:at * L + 2])   # the two symbols in front of symbol at * L
        assert b.quality_plan() == want_plan(source, sym[at:at + sz], front), f"{what}: plan of piece {k} (rows {at} .. {at + sz})"
        at += sz
        qp, f4 = reference(sym[:at], bases[:at], prev)
        assert np.array_equal(qp, sym[:at])
        same_table(b, 0, f4, prev, f"{what}: behind piece {k} ({at} rows)")
    same_symbols(b, 0, sym, what)
    return b


@functools.lru_cache(maxsize=None)
def l75_piece_sizes():
    """Pieces of 1, 2, 3, 5, 16 and 333 records in an order that starts a piece at every residue mod 16 (75 is odd)."""
    rng = np.random.default_rng(75)
    sizes, starts = [], set()
    while len(starts) < 16 or set(sizes) != {1, 2, 3, 5, 16, 333}:
        starts.add(sum(sizes) * 75 % 16)
        sizes.append(int(rng.choice([1, 2, 3, 5, 16, 333], p=[0.22, 0.22, 0.22, 0.22, 0.08, 0.04])))
    return tuple(sizes)


@pytest.mark.parametrize("A", [39, 80])
def test_pieces_flat_L75(A, ctx, ingest_mode):
    """L = 75, rows flat: an appended piece begins at base * 75, any residue mod 16, and the flat path loads 16 bytes from
    there on; its two symbols in front are the rows' last."""
    sizes = l75_piece_sizes()
    starts = {sum(sizes[:k]) * 75 % 16 for k in range(len(sizes))}
    assert starts == set(range(16)) and set(sizes) == {1, 2, 3, 5, 16, 333} and sum(sizes) * 75 <= 200000
    N = sum(sizes)
    r, c = np.arange(N)[:, None], np.arange(75)[None, :]
    sym = ((7 * r + 3 * c) % A).astype(np.uint8)
    run_pieces(ctx, sym, random_bases(N, 75), sizes, 1, what=f"L = 75, A = {A}")


@pytest.mark.parametrize("A", [39, 80])
def test_pieces_fused_L100(A, ctx, ingest_mode):
    """L = 100, fused rows, pieces whose first tile boundary (symbol 65536 = row 655, column 36) falls inside a row, between
    pieces of one row and of less than a tile."""
    sizes = (700, 1, 660, 39)
    assert all(sz * 100 > TILE and TILE % 100 != 0 for sz in (700, 660))
    N = sum(sizes)
    r, c = np.arange(N)[:, None], np.arange(100)[None, :]
    sym = ((7 * r + 3 * c) % A).astype(np.uint8)
    run_pieces(ctx, sym, random_bases(N, 100), sizes, 1, what=f"L = 100, A = {A}")


@pytest.mark.parametrize("L", [1, 2])
def test_pieces_one_record_each(L, ctx, ingest_mode):
    """One record of one or two symbols per piece: 0, 1, 2, ... symbols lie in front (tri_prev_k's three branches; with
    L = 1 the second piece takes one symbol from the rows and one from the caller, who carried none)."""
    sym = np.array([11, 50, 12, 49, 13, 48, 14, 47, 30, 30, 30, 30][:6 * L], dtype=np.uint8).reshape(6, L)
    run_pieces(ctx, sym, random_bases(6, L), (1,) * 6, 2, what=f"L = {L}")


@pytest.mark.parametrize("L", [100, 75])
def test_piece_widens_the_alphabet(L, ctx, ingest_mode):
    """Piece 1 spans ten symbols, piece 2 brings 0 and 79: the counters of piece 1 stay where the narrow layout put them."""
    rng = np.random.default_rng(L)
    sym = (30 + rng.integers(0, 10, size=(100, L))).astype(np.uint8)
    sym[0, :2], sym[49, -2:] = (30, 39), (39, 30)
    sym[70, 5], sym[80, 7] = 0, 79
    assert span(sym[:50]) == (30, 10) and span(sym[50:]) == (0, 80)
    b = run_pieces(ctx, sym, random_bases(100, L), (50, 50), 1, what=f"L = {L}")
    assert b.quality_plan() == (1, 0, 80, 1)


@pytest.mark.parametrize("L", [100, 75])
def test_piece_narrower_than_what_it_follows(L, ctx, ingest_mode):
    """Piece 1 ends on 79 and 0, piece 2 holds one symbol only: its first two trigrams begin with symbols that it does not
    contain, so the layout must cover them."""
    rng = np.random.default_rng(L + 1)
    sym = np.full((80, L), 40, dtype=np.uint8)
    sym[:40] = (20 + rng.integers(0, 30, size=(40, L))).astype(np.uint8)
    sym[39, -2:] = (79, 0)
    assert span(sym[40:]) == (40, 1) and tuple(sym[39, -2:]) == (79, 0)
    b = run_pieces(ctx, sym, random_bases(80, L), (40, 40), 1, what=f"L = {L}")
    assert b.quality_plan() == (1, 0, 80, 1)


# ---- f. qprev -------------------------------------------------------------------------------------------------------------

STATES = [(500, 500), (500, 7), (7, 500), (7, 79), (0, 0)]


def qprev_case(L, NP):
    sym = (20 + np.random.default_rng([L, NP]).integers(0, 40, size=(NP, L))).astype(np.uint8)
    return sym, random_bases(NP, L)


@pytest.mark.parametrize("L,NP", [(100, 300), (1, 50), (1, 2), (1, 1)])
@pytest.mark.parametrize("state", STATES)
def test_qprev_single(state, L, NP, ctx, ingest_mode):
    """The symbols carried in from an earlier shard (scalce_params.qprev, 500 = none) against the oracle started from that
    state; finish() raises nothing, so tri_expected -- n minus the symbols without two predecessors -- agrees, down to one
    and two symbols.  The layout covers the carried symbols."""
    sym, bases = qprev_case(L, NP)
    check_one_piece(ctx, [sym], [bases], [source_rule(L, True, False)], qprev=[state, NONE], what=f"{state}, {NP} x {L}")


@pytest.mark.parametrize("L,NP", [(100, 300), (1, 50)])
@pytest.mark.parametrize("i", range(len(STATES)))
def test_qprev_paired(i, L, NP, ctx, ingest_mode):
    """... paired, another state per mate."""
    s1, b1 = qprev_case(L, NP)
    s2, b2 = s1[::-1].copy(), random_bases(NP, L, seed=2)
    states = [STATES[i], STATES[(i + 1) % len(STATES)]]
    src = source_rule(L, False, False)
    check_one_piece(ctx, [s1, s2], [b1, b2], [src, src], qprev=states, what=f"{states}, {NP} x {L}")


def test_qprev_widens_the_layout(ctx, ingest_mode):
    """(7, 79) in front of a piece of nothing but 40: lo = 7, A = 73."""
    sym = np.full((300, 100), 40, dtype=np.uint8)
    b = check_one_piece(ctx, [sym], [random_bases(300, 100)], [1], qprev=[(7, 79), NONE], what="(7, 79) | 40 ...")
    assert b.quality_plan() == (1, 7, 73, 1)


def test_qprev_in_front_of_pieces(ctx, ingest_mode):
    """Carried symbols and pieces of one symbol each: the second piece has one symbol of the rows and one carried one in
    front (tri_prev_k: symbols_before == 1 takes carried1)."""
    sym = np.array([11, 50, 12, 49, 13, 48], dtype=np.uint8).reshape(6, 1)
    run_pieces(ctx, sym, random_bases(6, 1), (1,) * 6, 2, qprev=[(7, 79), NONE], what="(7, 79), L = 1")


# ---- g. one run end to end with the full alphabet -------------------------------------------------------------------------

def test_full_alphabet_end_to_end(ctx, oracle_trie, ingest_mode):
    """2000 x 100 with all 80 symbols through every stage: table, scaled table and coder bytes -- nothing behind the statistics
    assumes the 41 symbols of the usual inputs."""
    from gpu_util import hip_compress, oracle_streams
    sym, bases = uniform_case(0, 80, 2000, 100)
    quals = (sym + 33).astype(np.uint8)
    b = hip_compress(ctx, synth.fastq_bytes_fast(bases, quals), 100)
    ref = oracle_streams(oracle_trie, bases, quals)
    assert span(ref["qp"]) == (0, 80) and np.array_equal(ref["f4"], trigram_table(ref["qp"]))
    assert b.quality_plan() == (1, 0, 80, 1)
    same_table(b, 0, ref["f4"], what="end to end")
    same_symbols(b, 0, ref["qp"], what="end to end")
    table = b.output(host.OUT_TABLE, 0, np.uint32)
    assert np.array_equal(table, O.ac_scale(ref["f4"], 1)), "scaled table"
    assert np.array_equal(b.output(host.OUT_PERM, 0, np.uint32), ref["perm"]), "order"
    enc = b.output(host.OUT_QUAL, 0)
    want = O.AcStat(table).encode_stream(ref["qp"][ref["perm"]].reshape(-1))
    assert len(enc) == len(want), f"coder: {len(enc)} vs {len(want)} bytes"
    bad = np.flatnonzero(enc != want)
    assert len(bad) == 0, f"coder bytes differ first at {bad[:4]} of {len(want)}"
