"""scalce_range_plan_quality: which frames of the coded quality stream a range of records needs, how many symbols are
dropped in front of its first record and how many follow -- against a restatement in Python, at every frame boundary."""
import itertools

import pytest

from scalce_amd import host

FRAME = 10 * 1024 * 1024
LENGTHS = [1, 36, 64, 100, 150, 301, 1000, 2498]


def plan(L, first, n, total):
    """symbols [first * L, (first + n) * L) of `total` symbols in frames of FRAME; first / n clamped to the total // L records;
    the range that reaches the last record takes the symbols behind it along (a whole run decodes them)"""
    records = total // L
    first = min(first, records)
    n = records - first if n is None else min(n, records - first)
    if n == 0:
        return (first * L // FRAME, 0, 0, 0)
    s0 = first * L
    s1 = total if first + n == records else (first + n) * L
    f0 = s0 // FRAME
    return (f0, -(-s1 // FRAME) - f0, s0 - f0 * FRAME, s1 - s0)


def totals(L):
    """a stream of whole frames and one that ends inside its fourth frame, behind a last record and 0..L-1 more symbols"""
    return [3 * FRAME, 3 * FRAME + (FRAME // 3) // L * L + min(L - 1, 7)]


def edges(L, total):
    """record indices at 0, at 1, one record either side of every frame boundary, at the end and beyond it"""
    records = total // L
    pts = {0, 1, records - 1, records, records + 1, records + 1000}
    for f in range(1, -(-total // FRAME) + 1):
        r = f * FRAME // L
        pts.update({r - 1, r, r + 1})
    return sorted(p for p in pts if p >= 0)


@pytest.mark.parametrize("L", LENGTHS)
def test_plan_is_the_restatement_at_every_edge(L):
    for total in totals(L):
        e = edges(L, total)
        counts = [0, 1, 2, None] + [b - a for a, b in itertools.combinations(e, 2)]
        for first in e:
            for n in sorted(set(c for c in counts if c is not None)) + [None]:
                got = host.range_plan_quality(L, first, n, total)
                assert got == plan(L, first, n, total), (L, first, n, total)


@pytest.mark.parametrize("L", LENGTHS)
def test_plan_properties(L):
    for total in totals(L):
        records = total // L
        e = edges(L, total)
        for first in e:
            assert host.range_plan_quality(L, first, 0, total)[1:] == (0, 0, 0)          # n = 0: no frame
            for last in (p for p in e if p > first):
                f0, nf, dropped, decoded = host.range_plan_quality(L, first, last - first, total)
                assert f0 * FRAME + dropped + decoded <= total and dropped + decoded <= total
                assert dropped < FRAME
                if first < records:
                    # the launch: whole frames but the last, which holds at least one symbol of the range
                    assert (nf - 1) * FRAME < dropped + decoded <= nf * FRAME
                    assert decoded == (total - first * L if last >= records else (last - first) * L)
                # the range behind it: its frames begin where these end, or one frame sooner (a shared frame)
                g0, ng, _, _ = host.range_plan_quality(L, last, None, total)
                if first < records and last < records:
                    assert 0 <= f0 + nf - g0 <= 1, (L, first, last, total)
                    assert f0 + nf - g0 == (1 if last * L % FRAME else 0)
                    assert g0 + ng == -(-total // FRAME)


def test_plan_rejects_a_read_length_of_zero():
    with pytest.raises(host.ScalceError):
        host.range_plan_quality(0, 0, 1, FRAME)


def test_whole_run_is_the_range_from_zero_to_the_end():
    for L in LENGTHS:
        for total in totals(L) + [0, L - 1, L, FRAME + 1]:
            want = (0, -(-total // FRAME), 0, total) if total >= L else (0, 0, 0, 0)
            assert host.range_plan_quality(L, 0, None, total) == want, (L, total)
