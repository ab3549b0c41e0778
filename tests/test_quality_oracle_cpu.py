"""What test_gpu_quality_stats.py relies on, checked without a device: its numpy restatement of the trigram count against
the oracle (oraclelib.quality_stream, with and without carried symbols), and the claims its cases make about themselves."""
import numpy as np
import pytest

import oraclelib as O
import test_gpu_quality_stats as T


def streams():
    rng = np.random.default_rng(80)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = {
        "A80": rng.integers(0, 80, size=(400, 100)),
        "constant": np.full((50, 100), 40),
        "L1": rng.integers(0, 80, size=(300, 1)),
        "L2": rng.integers(0, 80, size=(300, 2)),
        "one_symbol": np.array([[9]]),
        "two_symbols": np.array([[9], [70]]),
        "L75_N": rng.integers(2, 41, size=(200, 75)),
    }
    cases = {}
    for name, sym in out.items():
        bases = acgt[rng.integers(0, 4, size=sym.shape)]
        if name == "L75_N":
            bases[3, 10] = bases[3, 11] = bases[199, 74] = ord("N")   # an N turns its q' into 0
        cases[name] = (sym.astype(np.uint8), bases)
    return cases


@pytest.mark.parametrize("prev", T.STATES + [(500, 0), (79, 79)])
@pytest.mark.parametrize("name", list(streams()))
def test_restatement_equals_oracle(name, prev):
    sym, bases = streams()[name]
    qp, f4 = O.quality_stream((sym + 33).astype(np.uint8), bases, 33, T.IDENT, prev=prev)
    if name == "L75_N":
        assert qp[3, 10] == 0 and qp[3, 11] == 0 and qp[199, 74] == 0 and T.span(qp) == (0, 41)
        sym = np.where(bases == ord("N"), 0, sym)
    assert np.array_equal(qp, sym)
    mine = T.trigram_table(qp, prev)
    assert np.array_equal(f4, mine), f"differ at {np.flatnonzero(f4 != mine)[:5]}"
    # one count per symbol with two predecessors, and the table that starts at 1 only where the mate begins
    n, have = qp.size, (2 if prev[0] < 256 and prev[1] < 256 else 1 if prev[1] < 256 else 0)
    start = 512000 if prev[1] >= 256 else 0
    assert int(f4.sum()) == start + max(0, n - (2 - have))


def test_default_prev_is_the_start_of_a_mate():
    sym, bases = streams()["A80"]
    a = O.quality_stream((sym + 33).astype(np.uint8), bases, 33, T.IDENT)
    b = O.quality_stream((sym + 33).astype(np.uint8), bases, 33, T.IDENT, prev=(500, 500))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].min() == 1


def test_pass_counts_of_the_layout():
    """61000 // A^2 leading symbols per pass: what the span cases claim, and where the last pass is short or `used` is odd."""
    assert [T.passes(A) for A in (1, 2, 39, 40, 41, 55, 79, 80)] == [1, 1, 1, 2, 2, 3, 9, 9]
    assert {A: T.passes(A) for _, A in T.SPANS} == T.PASSES
    assert T.FIELDS // 39 ** 2 >= 39 and T.FIELDS // 40 ** 2 < 40   # 39: the whole alphabet in one pass (the fast loop); 40: not
    for A in (40, 41, 55, 79, 80):                                    # the last pass holds fewer leading symbols
        assert T.layout(A)[-1] < T.layout(A)[0]
    for A in (1, 39, 41, 55, 79):                                     # an odd `used`: one live field in the last word
        assert any(u % 2 for u in T.layout(A))
    assert all(sum(T.layout(A)) == A ** 3 and max(T.layout(A)) <= T.FIELDS for A in range(1, 81))


def test_flat_shapes_cover_the_tails():
    sh = T.flat_shapes()
    for L in (1, 3, 15, 75, 161):   # odd lengths reach every residue
        assert {NP * L % 16 for l, NP in sh if l == L and NP * L >= 16} == {0, 1, 15}
    for L in (2, 8, 200):           # n is even: 1 and 15 cannot be left
        assert {NP * L % 16 for l, NP in sh if l == L and NP * L >= 16} == {0}
    assert all(any(l == L and NP * L < 16 for l, NP in sh) for L in (1, 2, 3, 8, 15))
    assert all(NP * L <= 200000 for L, NP in sh)


def test_l75_pieces_start_at_every_residue():
    sizes = T.l75_piece_sizes()
    assert {sum(sizes[:k]) * 75 % 16 for k in range(len(sizes))} == set(range(16))
    assert set(sizes) == {1, 2, 3, 5, 16, 333} and sum(sizes) * 75 <= 200000 and len(sizes) <= 64


@pytest.mark.parametrize("variant", ["constant", "ends_0_79", "period3"])
def test_guard_cases_pass_32768(variant):
    sym, bases, qp, f4, hot = T.guard_case(variant)
    assert int(f4.max()) - 1 > 32768 and qp.size <= 200000
    if variant != "period3":
        assert min(hot.values()) >= 32768   # inside ONE tile: one wave alone takes the field past the guard bit
