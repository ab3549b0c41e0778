"""The crafted texts of tests/test_gpu_ingest.py, built with ingest_ref's builder.  Every case says what it claims to be -- the
kernel it is named after, whether the one-pass kernel gives up first, where a chosen record starts and ends, which workgroups of
the tiled kernel read from LDS -- and tests/test_ingest_ref_cpu.py asserts those claims without a device, so that a text that
misses its edge fails there and does not pass silently on the GPU.

Variants of a text: "fastq" (single-end), "Q" (qualities dropped), "f" (two-line records), "i" (interleaved pairs: the records
of interest are mate 2's, mate 1 has another read length), "mate2" (two texts: the records of interest are mate 2's)."""
from dataclasses import dataclass, field

import numpy as np

import ingest_ref as R
import oraclelib as O

T = R.ING_TILE
W = R.ING_TILE + R.ING_OVER
VARIANTS = ("fastq", "Q", "f", "i", "mate2")


@dataclass
class Case:
    id: str
    texts: list                      # bytes, one per text
    L: tuple                         # read length per mate
    lpr: int = 4
    qout: bool = True                # q' rows are made (False: -Q, -f)
    il: bool = False
    use_names: bool = True
    qmap: list = None                # [(offset, values)] per mate, None = identity at 33
    no_ac: bool = False
    indexed: bool = False            # SCALCE_INGEST_INDEXED is set
    unfuse: bool = False             # set_fused_rows(False) first
    prefix: list = None              # texts ingested as a first piece, in front (append)
    kernel: int = 1                  # claimed: out[0] of the LAST mate (the records of interest)
    slow: int = 0                    # claimed: out[1]
    claims: list = field(default_factory=list)     # (text, record in the text, start or None, end or None)
    wg_in_lds: dict = None           # claimed: {workgroup of unpack_tiled_k: its text fits unp_text_cap} (single text)
    error: tuple = None              # claimed: (code, record, aux)
    text_bytes: int = None           # claimed: length of the last text
    span: tuple = None               # claimed: (lo, A) of the last mate's q'
    name_line_ends_behind: int = None   # claimed: the first claim's record ends its NAME line at or behind this offset

    def __repr__(self):
        return self.id


class Expect:
    """The restatement's word on a case, per mate"""
    pass


def expect(case, texts=None, indexed=None):
    """-> Expect: rows, bases, quals, qp, plan per mate; names, namelen; consumed per text; error; nrec"""
    texts = case.texts if texts is None else texts
    indexed = case.indexed if indexed is None else indexed
    maps = case.qmap or [R.IDENTITY_MAP] * len(case.L)
    kw = dict(lpr=case.lpr, use_names=case.use_names, qout=case.qout, no_ac=case.no_ac, indexed=indexed)
    if case.il:
        run = lambda take: [R.ingest(texts[0], case.L, interleave=True, qmap=maps, take=take, **kw)]   # noqa: E731
    else:
        run = lambda take: [R.ingest(t, case.L[m], mate=m, qmap=maps[m], take=take, **kw) for m, t in enumerate(texts)]   # noqa: E731
    outs = run(None)
    if len({o.nrec for o in outs}) > 1:   # the mates are read in step (compress.cpp:614-666): the common count
        outs = run(min(o.nrec for o in outs))
    e = Expect()
    e.outs, e.nrec, e.maps = outs, outs[0].nrec, maps
    flat = [(o, m) for o in outs for m in range(len(o.L))]
    e.rows, e.bases, e.quals, e.qp = ([getattr(o, k)[m] for o, m in flat] for k in ("rows", "bases", "quals", "qp"))
    e.plan = [o.plan[m] for o, m in flat]
    if not case.il and len(outs) == 2:    # mate 2's own text: no names of its own
        e.plan[1] = e.plan[1][:3] + (0,)
    e.names, e.namelen = outs[0].names, outs[0].namelen
    e.consumed = [o.consumed for o in outs]
    errs = [o.error for o in outs if o.error]
    e.error = errs[0] if errs else None
    return e


class Layout:
    """The records of one variant: `mine` are the records of interest (read length L), `other` mate 1's where there is one
    (read length Lo), `flat` the records of the text that holds `mine`, `named` the records whose names are stored."""

    def __init__(self, variant, L, n, seed, Lo=None, **kw):
        self.variant, self.L, self.n = variant, L, n
        self.lpr = 2 if variant == "f" else 4
        self.Lo = Lo or (40 if L != 40 else 24)
        self.mine = R.random_recs(n, L, seed, self.lpr, **kw)
        self.other = None
        if variant in ("i", "mate2"):
            self.other = R.random_recs(n, self.Lo, seed + 1000, self.lpr, name=lambda i: b"p%d" % i)
        self.flat = [r for pair in zip(self.other, self.mine) for r in pair] if variant == "i" else self.mine
        self.named = self.other if self.other is not None else self.mine

    def at(self, k):
        """where record k of `mine` is in `flat`"""
        return 2 * k + 1 if self.variant == "i" else k

    def nearest(self, offset):
        """the last record of `mine` that starts at or in front of `offset`"""
        offs = np.concatenate([[0], np.cumsum([len(r) for r in self.flat])])
        return max(k for k in range(self.n) if offs[self.at(k)] <= offset)

    def texts(self):
        mine = R.join(self.flat)
        return [R.join(self.other), mine] if self.variant == "mate2" else [mine]

    def case(self, id, prefix_n=0, **kw):
        single = self.variant in ("fastq", "Q", "f")
        c = Case(id=f"{id}-{self.variant}", texts=self.texts(), L=(self.L,) if single else (self.Lo, self.L), lpr=self.lpr,
                 qout=self.variant not in ("Q", "f"), il=self.variant == "i", **kw)
        if prefix_n:
            p = Layout(self.variant, self.L, prefix_n, 4242, Lo=self.Lo)
            for r in p.mine + (p.other or []):
                r.head = b"a" + r.head
            c.prefix = p.texts()
        return c

    def claim(self, k, start=None, end=None):
        return (1 if self.variant == "mate2" else 0, self.at(k), start, end)


def n_for(L, nbytes=40000):
    return int(min(1000, max(300, nbytes // (2 * L + 12))))


# ---- a. one-pass kernel, read lengths ---------------------------------------------------------------------------------------
LENGTHS = list(range(16, 34)) + [60, 61, 124, 125, 159, 160]   # every tail L % 16, both sides of the stride's steps, the ends


def length_cases():
    assert [R.row_stride(L) for L in (60, 61, 124, 125)] == [16, 32, 32, 48]   # the steps of stride[m] (batch_create)
    out = []
    for L in LENGTHS + [15, 161]:
        kernel = R.K_ONE_PASS if 16 <= L <= 160 else R.K_TILED if L < 16 else R.K_DIRECT
        for variant in ("fastq", "mate2"):
            out.append(Layout(variant, L, n_for(L), L).case(f"len{L}", kernel=kernel))
        if L % 4 == 0 and 16 <= L <= 160:   # (the batch picks fused rows for these: once more with rows back to back)
            out.append(Layout("fastq", L, n_for(L), L).case(f"len{L}_unfused", kernel=kernel, unfuse=True))
    return out


# ---- b. one-pass kernel, tile geometry --------------------------------------------------------------------------------------
GEO_L = 50
GEO_VARIANTS = ("fastq", "Q", "f", "i")


def geo_layout(variant, n=None):
    return Layout(variant, GEO_L, n or (260 if variant == "i" else 450 if variant != "f" else 800), 7)


def placed(variant, id, start, end=None, slow=0, n=None):
    lay = geo_layout(variant, n)
    k = lay.nearest(start)
    R.start_at(lay.flat, lay.at(k), start)
    if end is not None:
        R.end_at(lay.flat, lay.at(k), end)
    return lay.case(id, kernel=R.K_TILED if slow else R.K_ONE_PASS, slow=slow, claims=[lay.claim(k, start, end)])


def geometry_cases():
    out = []
    for v in GEO_VARIANTS:
        for d in (-2, -1, 0, 1):      # '@' as a tile's last byte (-1), a newline as its last byte (0: the record starts ON the tile)
            out.append(placed(v, f"start{T + d}", T + d))
        for b in (1, 2):              # at the first and the second tile boundary: the last newline on the overlap's last byte, and behind it
            out.append(placed(v, f"tile{b}_ends_on_last_overlap_byte", b * T - 1, b * T + R.ING_OVER - 1))
            out.append(placed(v, f"tile{b}_ends_behind_overlap", b * T - 1, b * T + R.ING_OVER, slow=1))
        # the NAME line begins in the tile and ends behind the overlap: no newline of the record is in its window
        lay = geo_layout(v)
        k = lay.nearest(T - 1)
        f = lay.at(k) - (1 if v == "i" else 0)      # (-i: the pair's first record, mate 1's)
        R.start_at(lay.flat, f, T - 1)
        lay.flat[f].pad_head(R.ING_OVER + 40)
        out.append(lay.case("name_line_leaves_the_window", kernel=R.K_TILED, slow=1,
                            claims=[(0, f, T - 1, None)], name_line_ends_behind=W))
        # the text ends inside the overlap: the record that starts on the tile's last byte is the text's last
        lay = geo_layout(v)
        k = lay.nearest(T - 1)
        R.start_at(lay.flat, lay.at(k), T - 1)
        del lay.flat[lay.at(k) + 1:]
        if lay.other is not None:
            del lay.other[k + 1:]
        lay.n = k + 1
        c = lay.case("text_ends_in_overlap", claims=[lay.claim(k, T - 1, None)])
        c.text_bytes = len(c.texts[-1])
        assert T < c.text_bytes < W
        out.append(c)
        for r in range(16):           # the last record ends on the text's last byte; the text's length at every residue mod 16
            lay = geo_layout(v, 150 if v == "i" else 300)
            size = (len(R.join(lay.flat)) + 63) // 64 * 64 + 64 + r - 8
            R.end_at(lay.flat, len(lay.flat) - 1, size - 1)
            c = lay.case(f"text_bytes_64k{r - 8:+d}", claims=[lay.claim(lay.n - 1, None, size - 1)])
            c.text_bytes = size
            out.append(c)
    # -i: mate 1 ends inside the tile, mate 2 beyond the overlap
    lay = geo_layout("i")
    k = lay.nearest(T - 1)
    R.start_at(lay.flat, lay.at(k), T - 1)          # mate 2 starts on the tile's last byte: mate 1 ends on the byte in front
    R.end_at(lay.flat, lay.at(k), T + R.ING_OVER + 5)
    out.append(lay.case("mate1_in_tile_mate2_behind_overlap", kernel=R.K_TILED, slow=1,
                        claims=[(0, 2 * k, None, T - 2), lay.claim(k, T - 1, T + R.ING_OVER + 5)]))
    return out


# ---- c. fallback ----------------------------------------------------------------------------------------------------------------
LONG_RECORD = W + 100    # a record of this many bytes leaves every window it starts in


def fallback_cases():
    out = []
    for v in VARIANTS:
        for where in ("first", "last", "boundary"):
            lay = Layout(v, 100, 150 if v == "i" else 300 if v != "f" else 500, 11)
            k = {"first": 0, "last": lay.n - 1, "boundary": lay.nearest(T - 1)}[where]
            start = None
            if where == "boundary":
                start = T - 1
                R.start_at(lay.flat, lay.at(k), start)
            lay.mine[k].pad(LONG_RECORD - len(lay.mine[k]))
            for pre in (0, 37):
                out.append(lay.case(f"long_record_{where}" + ("_appended" if pre else ""), prefix_n=pre, kernel=R.K_TILED, slow=1,
                                    claims=[lay.claim(k, start, None)]))
    return out


# ---- d. indexed tiled kernel ----------------------------------------------------------------------------------------------------
def tiled_cases():
    out = []
    for L in (1, 2, 3, 4, 5, 15):
        for n in (1, 127, 128, 129, 257):
            out.append(Layout("fastq", L, n, 100 * L + n).case(f"tiled_L{L}_n{n}", kernel=R.K_TILED))
    for v in VARIANTS:   # the switch, at a read length the one-pass kernel would take
        out.append(Layout(v, 100, 300, 13).case("indexed_by_switch", kernel=R.K_TILED, indexed=True))
    for long_wg in (0, 1):   # one workgroup's text beyond unp_text_cap (read from memory), the other's inside (from LDS)
        lay = Layout("fastq", 12, 256, 17)
        for r in lay.mine[128 * long_wg:128 * long_wg + 128]:
            r.pad(250)
        out.append(lay.case(f"text_cap_wg{long_wg}_from_memory", kernel=R.K_TILED, wg_in_lds={long_wg: False, 1 - long_wg: True}))
    out.append(Layout("fastq", 5, 200, 19).case("odd_L_at_odd_base_row", prefix_n=3, kernel=R.K_TILED))
    out.append(Layout("i", 40, 200, 23, Lo=12).case("only_mate2_in_16_160", kernel=R.K_TILED))
    out.append(Layout("i", 12, 200, 23, Lo=40).case("only_mate1_in_16_160", kernel=R.K_TILED))
    return out


# ---- e. direct kernel -------------------------------------------------------------------------------------------------------------
def direct_cases():
    out = []
    Ls, ns = (161, 255, 256, 300), (1, 255, 256, 257)
    for L in Ls:
        for n in ns:
            out.append(Layout("fastq", L, n, L + n).case(f"direct_L{L}_n{n}", kernel=R.K_DIRECT))
    for v in ("Q", "f", "i", "mate2"):
        for i, (L, n) in enumerate(zip(Ls, ns)):
            out.append(Layout(v, L, n, L + n, Lo=200 if i == 0 else None).case(f"direct_L{L}_n{n}", kernel=R.K_DIRECT))
    # (interleaved: the case above with mate 1 at 40 bases has the tiled kernel for mate 1 and this one for mate 2; here both)
    out.append(Layout("i", 170, 257, 71, Lo=165).case("direct_both_mates_n257", kernel=R.K_DIRECT))
    return out


# ---- f. names ---------------------------------------------------------------------------------------------------------------------
def name_heads():
    """name lines (behind their first byte): stored lengths 0 .. 255, the first space at every phase of the four-byte scan, no
    space at all, tabs and bytes >= 0x80, a 15-character name with a comment behind it"""
    heads = [b"", b" comment"]
    for n in (1, 3, 4, 5, 14, 15, 16, 17, 255):
        nm = bytes(65 + (i * 7 + n) % 26 for i in range(n))
        heads += [nm, nm + b" c", nm + b" a longer comment with spaces"]
    heads += [b"a\tb", b"\t", b"\x80\xff\xfe tail", b"tab\tand\x80high\xffbytes\tlonger", b"fifteen_chars_15 and a comment", b"x" * 15 + b" " + b"y" * 40]
    for n in range(6, 14):    # every phase, with the space as the line's last byte
        heads.append(b"n" * n + b" ")
    return heads


def names_layout(variant, n=300, L=36, seed=29):
    lay = Layout(variant, L, n, seed)
    heads = name_heads()
    for i, r in enumerate(lay.named):
        r.head = heads[(i + 3) % len(heads)] if i else b"fifteen_chars_15 first record"   # record 0: 15 characters and a comment
    for i, r in enumerate(lay.mine):          # a name without a space, then a sequence line whose first byte is a space
        if i % 9 == 4:
            r.seq = b" " + r.seq[1:]
    return lay


def name_cases():
    out = []
    for v in ("fastq", "f", "i"):
        out.append(names_layout(v).case("names", kernel=R.K_ONE_PASS))
        out.append(names_layout(v).case("names_indexed", kernel=R.K_TILED, indexed=True))
    out.append(names_layout("fastq").case("names_off", kernel=R.K_ONE_PASS, use_names=False))
    out.append(names_layout("fastq").case("names_off_indexed", kernel=R.K_TILED, indexed=True, use_names=False))
    out.append(names_layout("fastq", L=200).case("names_direct", kernel=R.K_DIRECT))
    c = names_layout("fastq").case("long_names_in_two_pieces", kernel=R.K_ONE_PASS)
    c.prefix = names_layout("fastq", n=120, seed=31).texts()
    out.append(c)
    c = names_layout("fastq").case("long_names_in_two_pieces_indexed", kernel=R.K_TILED, indexed=True)
    c.prefix = names_layout("fastq", n=120, seed=31).texts()
    out.append(c)
    return out


# ---- g. bytes -----------------------------------------------------------------------------------------------------------------------
NOT_NEWLINE = bytes(b for b in range(256) if b != 10)


def byte_layout(L, variant="fastq"):
    """255 records: every byte but the newline at every position of the sequence line, every character that maps to 0 .. 79 at
    every position of the quality line"""
    lay = Layout(variant, L, 255, 37)
    for r, rec in enumerate(lay.mine):
        rec.seq = bytes(NOT_NEWLINE[(r + 17 * p) % 255] for p in range(L))
        if rec.qual is not None:
            rec.qual = bytes(33 + (7 * r + 13 * p) % 80 for p in range(L))
    return lay


def lossy_map(text):
    """the table a lossy run samples from the text's quality lines (O.qmap_init): not the identity"""
    lines = text.split(b"\n")[3::4]
    stat = np.bincount(np.frombuffer(b"".join(lines), dtype=np.uint8), minlength=128)[:128]
    off, vals = O.qmap_init(stat, 30)
    assert not np.array_equal(vals, R.IDENT)
    return off, vals


def byte_cases():
    out = []
    for L in (16, 19):
        for indexed in (False, True):
            for lossy in (False, True):
                lay = byte_layout(L)
                c = lay.case(f"all_bytes_L{L}" + ("_table" if lossy else "_affine") + ("_indexed" if indexed else ""),
                             kernel=R.K_TILED if indexed else R.K_ONE_PASS, indexed=indexed)
                if lossy:
                    c.qmap = [lossy_map(c.texts[0])]
                out.append(c)
        out.append(byte_layout(L, "mate2").case(f"all_bytes_L{L}", kernel=R.K_ONE_PASS))
        out.append(byte_layout(L, "i").case(f"all_bytes_L{L}", kernel=R.K_ONE_PASS))
        out.append(byte_layout(L, "f").case(f"all_bytes_L{L}", kernel=R.K_ONE_PASS))
    # the largest symbol only as the last symbol of a tail unit (L = 19: units of 16 and 3)
    lay = Layout("fastq", 19, 500, 41, qlo=10, qhi=40, n_frac=0)
    lay.mine[333].qual = lay.mine[333].qual[:-1] + bytes([33 + 70])
    out.append(lay.case("largest_symbol_ends_a_tail_unit", span=(10, 61)))
    # the smallest character only under an N, which forces 0: 0 is the smallest symbol, the character's own is never seen
    lay = Layout("fastq", 19, 500, 43, qlo=10, qhi=40, n_frac=0)
    rec = lay.mine[222]
    rec.seq, rec.qual = rec.seq[:17] + b"N" + rec.seq[18:], rec.qual[:17] + bytes([33 + 3]) + rec.qual[18:]
    out.append(lay.case("smallest_symbol_under_an_N", span=(0, 41)))
    # the largest symbol only in the record that crosses a tile boundary
    lay = Layout("fastq", 50, 450, 47, qlo=10, qhi=40, n_frac=0)
    k, start = lay.nearest(T - 60), T - 60
    R.start_at(lay.flat, k, start)
    lay.mine[k].qual = lay.mine[k].qual[:-2] + bytes([33 + 70]) + lay.mine[k].qual[-1:]
    assert start + len(lay.mine[k]) - 3 > T     # the symbol lies in the next tile's text: only this record's workgroup sees it as a symbol
    out.append(lay.case("largest_symbol_in_the_crossing_record", span=(10, 61), claims=[lay.claim(k, start, None)]))
    return out


# ---- h. errors ------------------------------------------------------------------------------------------------------------------------
ERR_PATHS = {"one_pass": (40, R.K_ONE_PASS), "tiled": (12, R.K_TILED), "direct": (170, R.K_DIRECT)}
ERR_KINDS = ("seq_short", "seq_long", "qual_length", "name_256", "name_line_empty", "symbol_80", "symbol_79", "below_offset")
ERR_AT = 270   # of 280 records: not in the first workgroup of any kernel (the second tile of text, records 256 .. of the others)


def error_case(variant, path, kind, no_ac=False):
    L, kernel = ERR_PATHS[path]
    lay = Layout(variant, L, 280, 53, Lo=24 if path == "one_pass" else (8 if path == "tiled" else 161))
    rec, err = lay.mine[ERR_AT], None
    if kind == "seq_short":
        rec.seq, err = rec.seq[:-1], (R.E_READLEN, ERR_AT, L - 1)
    elif kind == "seq_long":
        rec.seq, err = rec.seq + b"A", (R.E_READLEN, ERR_AT, L + 1)
    elif kind == "qual_length":
        rec.qual, err = rec.qual + b"I", (R.E_READLEN, ERR_AT, L)     # (aux: the sequence line's length)
    elif kind == "name_256":
        lay.named[ERR_AT].head, err = b"n" * 256 + b" c", (R.E_NAMELEN, ERR_AT, 0)
    elif kind == "name_line_empty":
        lay.named[ERR_AT].head, lay.named[ERR_AT].lead, err = b"", b"", (R.E_NAMELEN, ERR_AT, 0)
    elif kind in ("symbol_80", "symbol_79", "below_offset"):
        ch = {"symbol_80": 33 + 80, "symbol_79": 33 + 79, "below_offset": 32}[kind]
        rec.qual = rec.qual[:L - 1] + bytes([ch])
        if rec.seq[L - 1:L] == b"N":
            rec.seq = rec.seq[:L - 1] + b"A"
        err = None if kind == "symbol_79" or no_ac else (R.E_SYMBOL, ERR_AT, 0)
    return lay.case(f"{kind}_{path}" + ("_no_ac" if no_ac else ""), kernel=kernel, error=err, no_ac=no_ac)


def error_cases():
    out = []
    for path in ERR_PATHS:
        for kind in ERR_KINDS:
            out.append(error_case("fastq", path, kind))
        for kind in ("symbol_80", "below_offset"):
            out.append(error_case("fastq", path, kind, no_ac=True))
        for kind in ("seq_short", "seq_long", "qual_length", "symbol_80", "below_offset"):
            out.append(error_case("mate2", path, kind))
        for kind in ERR_KINDS:
            out.append(error_case("i", path, kind))
    for kind in ("seq_short", "seq_long", "qual_length", "name_256", "name_line_empty"):
        out.append(error_case("Q", "one_pass", kind))
    for kind in ("seq_short", "seq_long", "name_256", "name_line_empty"):
        out.append(error_case("f", "one_pass", kind))
    return out


# ---- i. pieces ----------------------------------------------------------------------------------------------------------------------------
def piece_cases():
    """-> (id, case of the whole text, bytes of the first piece per text, what of them must be consumed)"""
    out = []
    lay = Layout("fastq", 50, 300, 59)
    whole = lay.case("pieces")
    text = whole.texts[0]
    start = R.offset_of(lay.flat, 200)
    nl = [start + i for i, b in enumerate(text[start:start + 400]) if b == 10]
    for name, cut in (("after_1_line", nl[0] + 1), ("after_2_lines", nl[1] + 1), ("after_3_lines", nl[2] + 1),
                      ("mid_line", nl[0] + 20), ("behind_a_record", start)):
        out.append((f"cut_{name}", whole, [cut], [start]))
    lay = Layout("mate2", 50, 300, 61)
    whole = lay.case("pieces")
    out.append(("mate1_ten_records_ahead", whole, [R.offset_of(lay.other, 210), R.offset_of(lay.mine, 200)],
                [R.offset_of(lay.other, 200), R.offset_of(lay.mine, 200)]))
    lay = Layout("i", 50, 300, 67)
    whole = lay.case("pieces")
    out.append(("cut_between_the_mates", whole, [R.offset_of(lay.flat, 2 * 150 + 1)], [R.offset_of(lay.flat, 2 * 150)]))
    return out


GROUPS = dict(lengths=length_cases, geometry=geometry_cases, fallback=fallback_cases, tiled=tiled_cases, direct=direct_cases,
              names=name_cases, bytes=byte_cases, errors=error_cases)
_CACHE = {}


def cases(group):
    if group not in _CACHE:
        _CACHE[group] = GROUPS[group]()
        ids = [c.id for c in _CACHE[group]]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return _CACHE[group]
