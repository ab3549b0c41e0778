"""The ingest stage restated in plain Python and numpy, and a builder of texts for it.  Nothing here knows of tiles, lanes or
workgroups except `predict_plan`, which restates from the kernels' comments WHEN the host leaves the one-pass kernel.

    text -> records (f_gets, compress.cpp:614-666) -> per mate: 2-bit rows (getval, const.cpp:47-49: C/c G/g T/t = 1 2 3, every
    other byte 0; four bases per byte, the first in bits 7-6), q' (output_quality, qualities.cpp:183, through the C oracle:
    exactly 'N' forces symbol 0), stored names (output_name, names.cpp:55-57: behind the line's first byte up to the first
    space or the newline), `consumed` = the offset behind the newline that ends the last record taken, the first error as
    (code, record, aux) in DevErrCode's meaning, and the plan scalce_batch_ingest_plan must report.

tests/test_ingest_ref_cpu.py holds all of it against the oracle and the golden vectors before any kernel is compared with it.
"""
import numpy as np

import oraclelib as O

# ---- the constants of the stage, as the kernels have them (scalce_amd/csrc/kernels_ingest.hpp) ------------------------------
IDX_TILE = 16384          # :53   IDX_THREADS * IDX_CHUNKS * 16
ING_TILE = IDX_TILE       # :409  text a workgroup of ingest_tiles2_k owns
ING_OVER = 1024           # :410  ... and what it reads behind it: the records that start in the tile must end there
ING_NLMAX = 2048          # :411  newlines a tile + overlap may hold
UNP_RPB = 128             # :333  records per workgroup of unpack_tiled_k
UNP_Q_CAP = 20 * 1024     # :334  UNP_RPB * L must fit: the tiled kernel up to L = 160, unpack_k beyond
ONE_PASS_L = (16, 160)    # piece_unpack_t, host_ingest.inc: `a.L >= 16 && a.L <= 160`
CELL_CHARS = 15           # a name cell is [length][15 characters]; longer names go to the long-name store
E_READLEN, E_NAMELEN, E_SYMBOL = 2, 3, 4                   # DevErrCode, :13-23
K_NONE, K_ONE_PASS, K_TILED, K_DIRECT = 0, 1, 2, 3        # scalce_batch_ingest_plan out[0]
MESSAGE = {E_READLEN: "read or quality line length differs from read_length (compress.cpp:628-634)",
           E_NAMELEN: "read name longer than 255 bytes or empty name line",
           E_SYMBOL: "quality symbol >= 80 after mapping (arithmetic.h:47)"}   # check_device_error, host_state.inc
IDENT = np.arange(128)
IDENTITY_MAP = (33, IDENT)

_CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in ((b"Cc", 1), (b"Gg", 2), (b"Tt", 3)):
    for _b in _c:
        _CODE[_b] = _v


def row_stride(L):
    """bytes between packed rows (batch_create, host_state.inc): the row's bytes and one spare zero byte, in 16s"""
    return ((L + 3) // 4 + 1 + 15) // 16 * 16


def unp_text_cap(L):
    """kernels_ingest.hpp:335: the text of a workgroup's 128 records that unpack_tiled_k copies to LDS; beyond it, it reads them
    from memory"""
    return ((UNP_RPB * (2 * L + 20) + 64) + 15) & ~15


def pack_rows(bases):
    """(n, L) bytes -> (n, ceil(L / 4)) 2-bit rows, zero behind the read"""
    bases = np.asarray(bases, dtype=np.uint8)
    n, L = bases.shape
    c = np.zeros((n, (L + 3) // 4 * 4), dtype=np.uint8)
    c[:, :L] = _CODE[bases]
    c = c.reshape(n, (L + 3) // 4, 4)
    return ((c[:, :, 0] << 6) | (c[:, :, 1] << 4) | (c[:, :, 2] << 2) | c[:, :, 3]).astype(np.uint8)


def stored_name(line):
    """output_name of one name line (without its newline): None for a line without a first byte"""
    if len(line) == 0:
        return None
    return line[1:].split(b" ", 1)[0]


def symbol_span(*parts):
    """(lo, A) of the symbols below 80 in the parts: what the trigram counters are laid out for"""
    s = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
    s = s[s < 80]
    return int(s.min()), int(s.max() - s.min() + 1)


class Ingested:
    """What one text becomes.  Per mate OF THE TEXT (one, or two under interleave): bases, quals (ASCII, n x L), rows, qp (None
    without qualities), plan; namelen / names: the first mate's, when the text is mate 1's."""
    pass


def lines_of(text):
    """offsets of the newlines"""
    return np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)


def ingest(text, L, lpr=4, interleave=False, mate=0, use_names=True, qout=True, qmap=None, no_ac=False, take=None, indexed=False):
    """text: bytes; L: the read length, (L1, L2) under interleave; lpr: lines per record (2: name and sequence only); mate: which
    mate's text this is when the mates come in two texts (names are mate 0's); qout: q' is made (False: -Q, and always with
    lpr = 2); qmap: (offset, values[128]), a pair of them under interleave; take: records (pairs) to take, None = every whole
    one; indexed: the caller has asked for the indexed kernels."""
    Ls = tuple(L) if interleave else (int(L),)
    nmate = len(Ls)
    maps = [IDENTITY_MAP] * nmate if qmap is None else (list(qmap) if interleave else [qmap])
    qout = qout and lpr == 4
    nl = lines_of(text)
    RL = lpr * nmate
    whole = len(nl) // RL
    n = whole if take is None else min(int(take), whole)
    out = Ingested()
    out.nrec, out.L, out.text_bytes, out.error = n, Ls, len(text), None
    out.consumed = int(nl[RL * n - 1]) + 1 if n else 0
    out.starts = [int(nl[RL * u - 1]) + 1 if u else 0 for u in range(n)]          # where unit u's name line begins
    out.ends = [int(nl[RL * u + RL - 1]) for u in range(n)]                      # the newline that ends its last line
    bases = [np.zeros((n, l), dtype=np.uint8) for l in Ls]
    quals = [np.zeros((n, l), dtype=np.uint8) for l in Ls]
    names, errors = [], []
    for u in range(n):
        for m in range(nmate):
            j = RL * u + lpr * m
            ns = int(nl[j - 1]) + 1 if j else 0
            ln = [text[ns:nl[j]]] + [text[nl[j + k - 1] + 1:nl[j + k]] for k in range(1, lpr)]
            if len(ln[1]) != Ls[m] or (lpr == 4 and len(ln[3]) != Ls[m]):
                errors.append((E_READLEN, u, len(ln[1])))        # aux: the length of the sequence line, as the kernels report it
                if m == 0 and mate == 0:
                    names.append(b"")
                continue
            bases[m][u] = np.frombuffer(ln[1], dtype=np.uint8)
            if lpr == 4:
                quals[m][u] = np.frombuffer(ln[3], dtype=np.uint8)
            if m == 0 and mate == 0:
                nm = stored_name(ln[0]) if use_names else b""
                if nm is None or len(nm) > 255:
                    errors.append((E_NAMELEN, u, 0))
                    nm = b""
                names.append(nm)
    out.bases, out.quals = bases, quals
    out.rows = [pack_rows(b) for b in bases]
    out.qp = [None] * nmate
    if qout:
        for m in range(nmate):
            off, vals = maps[m]
            out.qp[m] = O.quality_stream(quals[m], bases[m], off, vals, no_ac=True)[0]   # (no_ac: no counters; q' is the same)
            if not no_ac and not errors:
                bad = np.flatnonzero((out.qp[m] >= 80).any(axis=1))
                if len(bad):
                    errors.append((E_SYMBOL, int(bad[0]), 0))
    out.names = names if mate == 0 else None
    out.namelen = np.array([len(x) for x in names], dtype=np.uint8) if mate == 0 else None
    out.error = min(errors, key=lambda e: e[1]) if errors else None
    out.slow = predict_slow(text, nl, RL, n)
    out.plan = predict_plan(out, use_names and mate == 0, indexed)
    return out


def trigram_counts(out, m, maps=None):
    """the oracle's counter table of mate m's q' stream (+ 1 in every cell: qualities.cpp:191-196)"""
    off, vals = IDENTITY_MAP if maps is None else maps
    return O.quality_stream(out.quals[m], out.bases[m], off, vals)[1]


def windows(text_bytes):
    """[first byte, end) of what every workgroup of the one-pass kernel sees: piece t covers [16384 t, 16384 t + 17408), cut at the
    text's end"""
    return [(t * ING_TILE, min(t * ING_TILE + ING_TILE + ING_OVER, text_bytes)) for t in range((text_bytes + ING_TILE - 1) // ING_TILE)]


def predict_slow(text, nl, RL, take):
    """The rule of ingest_tiles2_k's comments (kernels_ingest.hpp:403-408, :532, :539-556): `slow` is raised if and only if a
    record (a pair under interleave) below the take count starts its name line in the first 16384 bytes of a piece and the newline
    that ends its last line is not inside that piece's window, or a window holds more than ING_NLMAX newlines."""
    n = len(text)
    for a, e in windows(n):
        if int(np.searchsorted(nl, e) - np.searchsorted(nl, a)) > ING_NLMAX:
            return True
    for u in range(take):
        ns = int(nl[RL * u - 1]) + 1 if u else 0
        a, e = windows(n)[ns // ING_TILE]
        if int(nl[RL * u + RL - 1]) >= e:
            return True
    return False


def predict_plan(out, names_on, indexed):
    """scalce_batch_ingest_plan of every mate of the text: (kernel, slow, line index built, long-name bytes)"""
    if out.nrec == 0:
        return [(K_NONE, 0, 0, 0)] * len(out.L)
    one_pass = all(ONE_PASS_L[0] <= l <= ONE_PASS_L[1] for l in out.L) and not indexed
    slow = one_pass and out.slow
    long_bytes = int(sum(len(x) for x in out.names if len(x) > CELL_CHARS)) if names_on and out.names is not None else 0
    if one_pass and not slow:
        kernels = [K_ONE_PASS] * len(out.L)
    else:
        kernels = [K_TILED if UNP_RPB * l <= UNP_Q_CAP else K_DIRECT for l in out.L]
    index = int(not (one_pass and not slow) or long_bytes > 0)
    return [(k, int(slow), index, long_bytes) for k in kernels]


# ---- the builder ---------------------------------------------------------------------------------------------------------
class Rec:
    """One record: `head` is the name line behind its first byte (name, and behind a space a comment), `plus` the comment of
    the '+' line; qual None: a two-line record."""

    def __init__(self, head, seq, qual=None, plus=b"", lead=b"@"):
        self.head, self.seq, self.qual, self.plus, self.lead = bytes(head), bytes(seq), None if qual is None else bytes(qual), bytes(plus), lead

    def bytes(self):
        r = self.lead + self.head + b"\n" + self.seq + b"\n"
        if self.qual is not None:
            r += b"+" + self.plus + b"\n" + self.qual + b"\n"
        return r

    def __len__(self):
        return len(self.bytes())

    def pad_head(self, d):
        """d more bytes of comment on the name line: the stored name stays what it is"""
        if d <= 0:
            assert d == 0
            return
        if b" " in self.head:
            self.head += b"x" * d
        else:
            self.head += b" " + b"x" * (d - 1)

    def pad(self, d):
        """d more bytes: half on the name line, half on the '+' line (all on the name line of a two-line record)"""
        if self.qual is None:
            self.pad_head(d)
        else:
            self.pad_head(d - d // 2)
            self.plus += b"y" * (d // 2)


def join(recs):
    return b"".join(r.bytes() for r in recs)


def offset_of(recs, k):
    return sum(len(r) for r in recs[:k])


def random_recs(n, L, seed, lpr=4, name=None, n_frac=0.01, qlo=2, qhi=40, lead=None):
    """n records of L bases: uniform ACGT with a few N, symbols uniform in [qlo, qhi] written at offset 33, names r<i>"""
    rng = np.random.default_rng([seed, n, L])
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))]
    bases[rng.random(size=(n, L)) < n_frac] = ord("N")
    quals = (33 + rng.integers(qlo, qhi + 1, size=(n, L))).astype(np.uint8)
    lead = lead or (b"@" if lpr == 4 else b">")
    return [Rec(name(i) if name else b"r%d" % i, bases[i].tobytes(), quals[i].tobytes() if lpr == 4 else None, lead=lead) for i in range(n)]


def start_at(recs, k, offset, most=120):
    """Comments on the name lines of the records in front of record k until it starts at `offset`: at most `most` bytes each, the
    nearest records first, so that none of them grows long"""
    need = offset - offset_of(recs, k)
    assert 0 <= need <= most * k, f"record {k} starts at {offset_of(recs, k)}: cannot be moved to {offset}"
    j = k - 1
    while need:
        d = min(need, most)
        recs[j].pad_head(d)
        need -= d
        j -= 1
    assert offset_of(recs, k) == offset


def end_at(recs, k, offset):
    """Comments on record k's own name and '+' lines until the newline that ends it is text byte `offset`"""
    need = offset - (offset_of(recs, k) + len(recs[k]) - 1)
    assert need >= 0
    recs[k].pad(need)
    assert offset_of(recs, k) + len(recs[k]) - 1 == offset
