"""tests/coder_totals.py held to its own claims, with the oracle alone: every case sums to its total, round-trips through the
oracle's coder (collapse: provably does not), and holds the steps it was crafted for -- so that the comparisons of
test_gpu_coder_totals.py cannot pass on inputs that never reach the edge they are named after."""
import numpy as np
import pytest

import coder_totals as T
import oraclelib as O

IDS = ["%s-%d" % c for c in T.CASES]


@pytest.mark.parametrize("name,total", T.CASES, ids=IDS)
def test_rows_sum_to_the_stated_total(name, total):
    c = T.case(name, total)
    assert c.table.dtype == np.uint32 and c.table.shape == (512000,) and c.table.min() >= 1
    sums = c.table.reshape(T.NCTX, T.AC_D).astype(np.int64).sum(axis=1)
    assert int(sums.max()) == total
    assert 20_000 <= len(c.sym) <= 70_000 and int(c.sym.max()) < T.AC_D
    visited = np.unique(c.sym[:-2].astype(np.int64) * T.AC_D + c.sym[1:-1])   # the contexts a symbol is coded in
    if name == "mixed":
        assert set(int(s) for s in sums) == set(T.MIXED_TOTALS) | {total}
        for t in T.MIXED_TOTALS + (total,):   # the maximum too sits in contexts that occur, often
            at = np.isin(c.sym[:-2].astype(np.int64) * T.AC_D + c.sym[1:-1], np.flatnonzero(sums == t))
            assert at.sum() >= 1000, (t, int(at.sum()))
    else:
        assert (sums == total).all()
        assert len(visited) >= len(c.frequent) ** 2


@pytest.mark.parametrize("name,total", [c for c in T.CASES if c[0] != "collapse"], ids=[i for i in IDS if "collapse" not in i])
def test_the_oracle_decodes_what_it_coded(name, total):
    c = T.case(name, total)
    st = O.AcStat(c.table)
    coded = st.encode_stream(c.sym)
    assert len(coded) == 4 + int.from_bytes(coded[:4].tobytes(), "little")   # one frame
    back = st.decode_block(coded[4:], len(c.sym))
    assert (back == c.sym).all(), f"first difference at symbol {np.flatnonzero(back != c.sym)[:4]}"


@pytest.mark.parametrize("name,total", [c for c in T.CASES if c[0] != "collapse"], ids=[i for i in IDS if "collapse" not in i])
def test_the_crafted_steps_are_there(name, total):
    """the rare symbols occur, with a count of 1 (floor) or thin_count (narrow, top_symbol); the narrow steps gave them the
    smallest intervals the total allows; the straddle stretch reaches more than 64 pending bits"""
    c = T.case(name, total)
    row0 = c.table.reshape(T.NCTX, T.AC_D)
    for s in c.rare:
        want = T.thin_count(total) if s == 36 else 1
        assert (row0[:, s] == want).all() and (c.sym == s).sum() >= 100, s
    for s in c.frequent:
        assert (row0[:, s] > T.thin_count(total)).all() and (c.sym == s).sum() >= 100, s
    w = c.widths
    assert 0 not in w, "an empty interval: the stream would not decode"
    if name != "mixed":
        assert c.maxpend > 64
        assert c.crafted == T.N_NARROW + T.N_STRADDLE
    if name in ("floor_inside", "floor_outside", "wide_span"):
        if total in (2 ** 29, 2 ** 29 + 1):
            assert w.get(2, 0) >= 100 and min(w) == 2, w   # two values: the least the plain step's exit test allows
        if total == 2 ** 29 - 1:
            assert w.get(2, 0) >= 100 and min(w) == 2, w
        if total >= 2 ** 30 - 1:
            assert w.get(1, 0) >= 100 and min(w) == 1, w   # one value: all 32 bits of lo and hi agree
    if name == "mixed":
        assert w.get(2, 0) >= 50 and min(w) == 2, w
    if name in ("narrow", "top_symbol") and total >= 2 ** 31:
        assert w.get(1, 0) >= 100 and min(w) == 1, w       # the thin symbol: width 1 in a stream that decodes


@pytest.mark.parametrize("total", [2 ** 29, 2 ** 29 + 1])
def test_wide_span_leaves_symbols_outside_the_decoder_cache(total):
    """host_decode.inc:57-58 restated (coder_totals.decoder_cache_width): fewer symbols are cached than are frequent, and
    those of rank W or above occur"""
    c = T.case("wide_span", total)
    W, order = T.decoder_cache_width(c.table)
    assert set(order) == set(c.frequent) and 1 < W < len(c.frequent), (W, len(order))
    assert np.isin(c.sym, order[W:]).sum() >= 1000
    assert np.isin(c.sym, order[:W]).sum() >= 1000
    for name in ("narrow", "floor_inside", "floor_outside", "mixed"):   # the others cache every frequent symbol
        other = T.case(name, total)
        W, order = T.decoder_cache_width(other.table)
        assert W == len(order) and set(other.frequent) <= set(order), name


def test_floor_symbols_lie_where_the_case_says():
    """inside or outside the span of the decoder's compact rows: smin .. smax of the symbols with a count above 1"""
    for name, inside in (("floor_inside", True), ("floor_outside", False), ("wide_span", True), ("mixed", True)):
        c = T.case(name, 2 ** 29)
        occ = np.flatnonzero((c.table.reshape(T.NCTX, T.AC_D) > 1).any(axis=0))
        assert all((occ.min() < s < occ.max()) == inside for s in c.rare), name
    c = T.case("top_symbol", 2 ** 29)
    assert (c.table.reshape(T.NCTX, T.AC_D)[:, 79] > 1).all() and (c.sym == 79).sum() >= 1000


@pytest.mark.parametrize("total", [3_000_000_078, 2 ** 32 - 1])
def test_collapse_pins_the_limit_of_the_format(total):
    """Above a context total of 2^30 a symbol at the floor count can receive an empty interval in the reference's 32-bit
    coder, and the reference's own decoder does not get the input back.  k is where it first fails."""
    c = T.case("collapse", total)
    st = O.AcStat(c.table)
    back = st.decode_block(st.encode_stream(c.sym)[4:], len(c.sym))
    bad = np.flatnonzero(back != c.sym)
    assert len(bad) and int(bad[0]) == c.k and c.k >= 64
    assert len(bad) > (len(c.sym) - c.k) // 4, "behind the first wrong symbol the stream is lost"
    assert np.isin(c.sym[:c.k], c.rare).any(), "floor-count symbols in front of k decode: not every one collapses"
    assert (c.table.reshape(T.NCTX, T.AC_D)[:, list(c.rare)] == 1).all()
    assert (st.decode_block(st.encode_stream(c.sym[:c.k])[4:], c.k) == c.sym[:c.k]).all()   # what the GPU test decodes


@pytest.mark.parametrize("name,total", [("floor_inside", 2 ** 30), ("narrow", 2 ** 32 - 1), ("collapse", 2 ** 32 - 1), ("mixed", 2 ** 29)])
def test_coder_step_is_the_oracles(name, total):
    """Coder, the reference's step restated in Python integers, against the oracle's coder: every turn of the renormalisation
    loop is one bit of the code (at once or as a pending bit), and flush adds two -- so the size of the oracle's block of the
    first n symbols is 2 raw bytes + ceil((turns + 2) / 8), for every n tried, inverted intervals included"""
    c = T.case(name, total)
    cum = T.cum_of(c.table.reshape(T.NCTX, T.AC_D)).tolist()
    st = O.AcStat(c.table)
    coder = T.Coder()
    coder.prev = (int(c.sym[0]), int(c.sym[1]))
    sizes = {}
    for i in range(2, 3000):
        row = cum[coder.prev[0] * T.AC_D + coder.prev[1]]
        coder.code(int(c.sym[i]), row, row[-1])
        sizes[i + 1] = 2 + (coder.shifts + 2 + 7) // 8
    for n in list(range(3, 200)) + [500, 1000, 2999, 3000]:
        assert len(st.encode_block(c.sym[:n])) == sizes[n], n


def test_craft_straddle_is_what_its_callers_had():
    """craft_straddle moved from gpu_util.py onto Coder: for the arguments of its callers (test_gpu_parity, test_gpu_coder_rounds)
    it returns what the version it replaced returned -- digests and pending runs recorded from that version"""
    import hashlib

    def digest(a):
        return hashlib.sha256(np.asarray(a).tobytes()).hexdigest()[:16]
    row = np.ones(80, dtype=np.uint32)
    row[8:40] = 1000
    cum = np.concatenate([[0], np.cumsum(row)])
    rng = np.random.default_rng(4)
    got = [T.craft_straddle(60_000, cum, int(cum[-1]), rng) for _ in range(2)]
    assert [(digest(p), m) for p, m in got] == [("63388f975a61f57f", 275), ("0ccdfea0ed01053e", 261)]
    p, m = T.craft_straddle(40_000, cum, int(cum[-1]), np.random.default_rng(11))
    assert (digest(p), m) == ("5aefbb5afe195e39", 284)
    row = np.ones(80, dtype=np.uint32)
    row[8:40] = 509
    row[8] += 49
    row[79] = 1 << 14
    cum = np.concatenate([[0], np.cumsum(row)])
    rng = np.random.default_rng(41)
    p, m = T.craft_straddle(40_000, cum, int(cum[-1]), rng, first2=(79, 79))
    assert (digest(p), m) == ("4707249e0b8a3889", 199)
    assert digest(rng.integers(0, 1 << 30, 8)) == "ea7b1c2b1dbf199e"   # and it drew as many numbers
