"""Tables and symbols at context totals of 2^29 to 2^32 - 1, for tests/test_coder_totals_cpu.py and
tests/test_gpu_coder_totals.py.

numpy, Python integers and (for the one figure of the collapse cases) the oracle; no GPU.  Every numeric precondition of
the coder kernels is a statement about the largest context total of the scaled table (2^29: the plain step of the encoders
and ac_decode_tight_k; 2^30: the reference's 32-bit intervals start to invert), so the cases stand on both sides of each.  What a case claims about itself -- which interval
widths its rare symbols received, how long its pending-underflow runs are, which symbols fall outside the decoder's LDS
cache -- is asserted with the oracle alone in test_coder_totals_cpu.py, so that a GPU comparison on it cannot pass emptily.

The generators follow the reference coder's registers symbol by symbol (Coder: arithmetic.cpp:122-152 in Python integers)
and choose the next symbol by what they see there."""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

M32 = 0xFFFFFFFF
AC_D = 80
NCTX = AC_D * AC_D
TOTALS = (2 ** 29 - 1, 2 ** 29, 2 ** 29 + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31, 3_000_000_078, 2 ** 32 - 1)
SLACK = 1 << 27              # craft_narrow: a rare symbol goes out whenever the range is at most 2^30 + SLACK
FREQUENT = (30, 31, 32, 40)
WEIGHTS = (0.4, 0.3, 0.2, 0.1)
N_NARROW, N_STRADDLE, N_RANDOM = 20_000, 15_000, 10_000   # symbols per stretch: a frame of 45 000
DEC_CACHE_ENTRIES = 19968    # AC_DEC_CACHE_ENTRIES, kernels_ac.hpp


def seed_of(case, *args):
    return zlib.crc32(("%s:%s" % (case, ",".join(map(str, args)))).encode())


def row_with(total, alphabet, weights, thin=()):
    """80 counts, all at least 1, that sum to exactly `total`: ones, the (symbol, count) pairs of `thin`, and what is left
    shared among `alphabet` by `weights` (the remainder of the rounding goes to its first symbol)"""
    row = np.ones(AC_D, dtype=np.int64)
    for s, c in thin:
        row[s] = c
    rest = int(total) - int(row.sum())
    w = np.asarray(weights, dtype=np.float64)
    add = np.floor(w / w.sum() * rest).astype(np.int64)
    add[0] += rest - int(add.sum())
    assert rest >= 0 and (add >= 0).all()
    row[np.asarray(alphabet)] += add
    assert int(row.sum()) == total and row.min() >= 1 and row.max() <= M32
    return row.astype(np.uint32)


def cum_of(rows):
    """cumulative counts with a leading 0 along the last axis: [.., 81]"""
    rows = np.asarray(rows, dtype=np.int64)
    return np.concatenate([np.zeros(rows.shape[:-1] + (1,), dtype=np.int64), np.cumsum(rows, axis=-1)], axis=-1)


class Coder:
    """The registers of the reference coder (ac_coder::write, arithmetic.cpp:122-152): lo and hi in 32 bits, the bounds
    from range + 1 in 64, the renormalisation and underflow loop.  pend: underflow bits pending; peak: the most that were
    pending at once since it was last set to zero; shifts: turns of the loop so far, each of which is one bit of the code.
    prev: the two symbols in front (None: nothing coded yet)."""

    def __init__(self):
        self.lo, self.hi, self.pend, self.peak, self.shifts, self.prev = 0, M32, 0, 0, 0, None

    def width(self):
        return ((self.hi - self.lo) & M32) + 1

    def bounds(self, c_lo, c_hi, total):
        """(lo, hi) of the symbol with cumulative counts [c_lo, c_hi) before the renormalisation, as the 32-bit registers
        hold them: hi = lo - 1 is an empty interval, the coder goes on with it all the same"""
        w = self.width()
        return (self.lo + w * int(c_lo) // int(total)) & M32, (self.lo + w * int(c_hi) // int(total) - 1) & M32

    def step(self, c_lo, c_hi, total):
        nl, nh = self.bounds(c_lo, c_hi, total)
        while True:
            if (nh & 0x80000000) == (nl & 0x80000000):
                self.pend = 0
            elif not (nh & 0x40000000) and (nl & 0x40000000):
                nl &= 0x3FFFFFFF
                nh |= 0x40000000
                self.pend += 1
                self.peak = max(self.peak, self.pend)
            else:
                break
            nl = (nl << 1) & M32
            nh = ((nh << 1) | 1) & M32
            self.shifts += 1
        self.lo, self.hi = nl, nh

    def code(self, s, cum, total):
        self.step(cum[s], cum[s + 1], total)
        self.prev = (self.prev[1], s)


def craft_straddle(n, cum, total, rng, first2=(9, 12), used=None, run_max=40, coder=None):
    """n symbols for a context-free table (cum[0..80] cumulative counts) chosen while following the reference coder's
    state (arithmetic.cpp:122-152): runs of 1..run_max symbols whose interval holds the midpoint -- each adds pending
    underflow bits -- between stretches of random symbols.  used: the symbols to choose from (default: every count above
    1).  coder: a Coder that has coded the symbols in front of the stretch (default: the start of a block, and the stretch
    begins with the two raw symbols first2).  Returns (symbols, longest pending run in bits)."""
    if coder is None:
        coder = Coder()
    out = []
    if coder.prev is None:
        out = [first2[0], first2[1]]
        coder.prev = (first2[0], first2[1])
    coder.peak = 0
    if used is None:
        used = [s for s in range(80) if cum[s + 1] > cum[s] + 1]
    used = list(used)
    run_left, free = 0, 0
    while len(out) < n:
        if run_left == 0 and free == 0:
            run_left, free = int(rng.integers(1, run_max + 1)), int(rng.integers(1, 12))
        pick = None
        if free == 0:
            for s in used:
                nl, nh = coder.bounds(cum[s], cum[s + 1], total)
                if 0x40000000 <= nl < 0x80000000 <= nh < 0xC0000000:
                    pick = s
                    break
            run_left -= 1
        if pick is None:
            pick = int(rng.choice(used))
            free = max(0, free - 1)
        coder.code(pick, cum, total)
        out.append(pick)
    return np.array(out[:n], dtype=np.uint8), coder.peak


def craft_narrow(n, cum, total, rng, floor_syms, slack=SLACK, first2=FREQUENT[:2], coder=None):
    """n symbols chosen while following the reference coder's state: one of floor_syms whenever the range is at most
    2^30 + slack -- so that the rarest symbols receive the smallest intervals the table allows --, else a random one of the
    other symbols with a count above 1.  cum: [81] cumulative counts of a context-free table (`total` its last entry), or
    [6400][81], one row per context (`total` is not read).  coder, first2: as for craft_straddle.
    Returns (symbols, {interval width: how many steps of a floor symbol received it}); width 0 is an empty interval."""
    cum = np.asarray(cum)
    if coder is None:
        coder = Coder()
    out = []
    if coder.prev is None:
        out = [first2[0], first2[1]]
        coder.prev = (first2[0], first2[1])
    floor_syms = [int(s) for s in floor_syms]
    hist, rows = {}, {}
    while len(out) < n:
        ctx = coder.prev[0] * AC_D + coder.prev[1] if cum.ndim == 2 else 0
        if ctx not in rows:
            c = [int(x) for x in (cum[ctx] if cum.ndim == 2 else cum)]
            rows[ctx] = (c, [s for s in range(AC_D) if c[s + 1] > c[s] + 1 and s not in floor_syms])
        c, used = rows[ctx]
        tot = c[AC_D] if cum.ndim == 2 else int(total)
        if coder.width() <= (1 << 30) + slack:
            s = floor_syms[int(rng.integers(0, len(floor_syms)))]
            nl, nh = coder.bounds(c[s], c[s + 1], tot)
            w = (nh - nl + 1) & M32
            hist[w] = hist.get(w, 0) + 1
        else:
            s = used[int(rng.integers(0, len(used)))]
        coder.code(s, c, tot)
        out.append(s)
    return np.array(out[:n], dtype=np.uint8), hist


# ---- the cases ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    total: int               # the largest context total of the table
    table: np.ndarray        # uint32[512000]
    sym: np.ndarray          # uint8, one frame
    frequent: tuple          # the symbols with large counts
    rare: tuple              # the symbols of the crafted narrow steps and of the 2 % in the random stretch
    widths: dict = field(default_factory=dict)   # craft_narrow's histogram
    maxpend: int = 0         # craft_straddle's longest pending run
    crafted: int = 0         # the frame's first `crafted` symbols are the crafted stretches
    k: int = -1              # collapse: index of the first symbol the oracle's own decoder gets wrong


def thin_count(total):
    """the smallest count above 1 whose interval cannot be empty: count * range / total >= 1 for every range the
    renormalisation leaves (above 2^30)"""
    return max(2, -(-total // (1 << 30)))


CASES = ([("narrow", t) for t in TOTALS] + [("floor_inside", t) for t in TOTALS[:6]] +
         [("floor_outside", t) for t in (2 ** 29, 2 ** 29 + 1)] + [("wide_span", t) for t in (2 ** 29, 2 ** 29 + 1)] +
         [("mixed", t) for t in (2 ** 29, 2 ** 29 + 1)] + [("top_symbol", t) for t in (2 ** 29, 2 ** 31)] +
         [("collapse", t) for t in (3_000_000_078, 2 ** 32 - 1)])
WIDE = tuple(s for s in range(20, 60) if s not in (33, 35))    # 38 frequent symbols, weights falling with the symbol
MIXED_TOTALS = (104, 2 ** 20)                                   # and the case's maximum


def random_stretch(rng, n, frequent, weights, rare, rare_frac=0.02):
    sym = rng.choice(np.asarray(frequent), size=n, p=np.asarray(weights) / np.sum(weights)).astype(np.uint8)
    if rare:
        at = np.flatnonzero(rng.random(n) < rare_frac)
        sym[at] = rng.choice(np.asarray(rare), size=at.size)
    return sym


def mixed_rows(total):
    """a total per context from {104, 2^20, total}: at random, but the 16 contexts of two frequent symbols -- the ones the
    symbols visit most -- take turns, so that each total is visited"""
    rng = np.random.default_rng(seed_of("mixed_rows", total))
    totals = (MIXED_TOTALS + (total,))
    pick = rng.integers(0, 3, size=NCTX)
    for i, (a, b) in enumerate((a, b) for a in FREQUENT for b in FREQUENT):
        pick[a * AC_D + b] = (i + 2) % 3
    one = [row_with(t, FREQUENT, WEIGHTS) for t in totals]
    return np.stack([one[p] for p in pick]), pick


@functools.lru_cache(maxsize=None)
def case(name, total):
    """narrow: four frequent symbols and a thin one (36, thin_count(total): the smallest intervals a stream that decodes can
      hold at this total), every context the same row.
    floor_inside: symbols 33 and 35 at the floor count 1, inside the span 30 .. 40 of the decoder's compact rows, occur.
    floor_outside: 5 and 70, outside the span.
    wide_span: 38 frequent symbols 20 .. 59, more than the decoder caches; 33 and 35 at the floor count.
    mixed: a total of 104, 2^20 or `total` per context (mixed_rows); 33 and 35 at the floor count.
    top_symbol: symbol 79 is frequent; a thin symbol as in narrow, and below 2^30 the floor symbols of floor_inside.
    collapse: narrow's frequent symbols, 2 % of the symbols at the floor count, above 2^30: the reference cannot decode it.
    Every frame but collapse's: a craft_narrow stretch on the rare symbols, a craft_straddle stretch on the frequent ones
    (not in mixed, whose contexts differ), random draws with 2 % rare symbols."""
    rng = np.random.default_rng(seed_of(name, total))
    frequent, weights, thin, rare = FREQUENT, WEIGHTS, (), (33, 35)
    if name == "narrow":
        thin, rare = ((36, thin_count(total)),), (36,)
    elif name == "floor_outside":
        rare = (5, 70)
    elif name == "wide_span":
        frequent, weights = WIDE, tuple(float(len(WIDE) + 4 - i) for i in range(len(WIDE)))
    elif name == "top_symbol":
        frequent = (30, 31, 32, 79)
        thin, rare = ((36, thin_count(total)),), ((36, 33, 35) if total < 2 ** 30 else (36,))
    elif name not in ("floor_inside", "mixed", "collapse"):
        raise KeyError(name)
    if name == "mixed":
        rows, _ = mixed_rows(total)
        cum = cum_of(rows)
    else:
        row = row_with(total, frequent, weights, thin)
        rows = np.tile(row, (NCTX, 1))
        cum = cum_of(row)
    table = np.ascontiguousarray(rows.reshape(-1), dtype=np.uint32)
    c = Case(name, total, table, None, tuple(frequent), tuple(rare))
    if name == "collapse":
        c.sym = np.concatenate([np.array(frequent[:2], dtype=np.uint8), random_stretch(rng, 30_000, frequent, weights, rare)])
        c.k = first_wrong(c)
        return c
    coder = Coder()
    first2 = (frequent[0], frequent[1])
    narrow, c.widths = craft_narrow(N_NARROW, cum, total, rng, rare, SLACK, first2, coder)
    parts = [narrow]
    if name != "mixed":
        straddle, c.maxpend = craft_straddle(N_STRADDLE, cum, total, rng, used=frequent, run_max=400, coder=coder)
        parts.append(straddle)
    c.crafted = sum(len(p) for p in parts)
    parts.append(random_stretch(rng, N_RANDOM, frequent, weights, rare))
    c.sym = np.concatenate(parts)
    return c


def first_wrong(c):
    """index of the first symbol that the oracle's decoder gets wrong in the oracle's own code of the frame; -1: none"""
    import oraclelib as O
    st = O.AcStat(c.table)
    back = st.decode_block(st.encode_stream(c.sym)[4:], len(c.sym))
    bad = np.flatnonzero(back != c.sym)
    return int(bad[0]) if len(bad) else -1


def decoder_cache_width(table):
    """(W, the symbols by rank) by the rule of scalce_ac_decoder_create (host_decode.inc:40-58): the span of the symbols
    with a count above 1 in some context, ranked by their totals over all contexts (stable), and as many of them cached as
    (W + 1)^2 rows of the span fit DEC_CACHE_ENTRIES, at most 32"""
    t = np.asarray(table, dtype=np.int64).reshape(NCTX, AC_D)
    tot = np.where(t > 1, t, 0).sum(axis=0)
    occ = np.flatnonzero(tot)
    s1 = int(occ.max()) - int(occ.min()) + 2
    order = sorted((int(s) for s in occ), key=lambda s: -int(tot[s]))
    w = 1
    while w < 32 and w < len(order) and (w + 1) * (w + 1) * s1 <= DEC_CACHE_ENTRIES:
        w += 1
    return w, order
