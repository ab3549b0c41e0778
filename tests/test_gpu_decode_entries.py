"""-m gpu: the two device entries behind windowed decompression, called directly -- scalce_ac_decoder_launch (runs of whole
frames from any frame of the stream into any byte address) and scalce_fastq_records_window (a window-relative directory,
names, qualities, offsets, and the archive-wide index of its first record) -- against tests/decode_ref.py, bit for bit.
Every output lies between guard bytes that must stay as they were, and is filled with a sentinel that must be gone;
an input tensor ends 64 bytes behind its data -- the slack the product guarantees behind reads, names and coded frames --
and those bytes are not zero."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as R
import oraclelib as O
from gpu_util import DEV, GUARD, SENT, In, Out  # noqa: F401
from scalce_amd import host

pytestmark = pytest.mark.gpu
FRAME = R.FRAME


@pytest.fixture(scope="module")
def ctx():
    return host.Context(0, patterns_text=CORE_TEXT)


# ---- device buffers: Out and In, between guard bytes (gpu_util) -----------------------------------------------------------
def dev_u64(values):
    import torch
    return torch.tensor([int(v) - (1 << 64) if int(v) >= 1 << 63 else int(v) for v in values], dtype=torch.int64, device=DEV)


# ---- decoder: tables (the shapes of test_decoder_compact_rows_and_lds_cache) ---------------------------------------------
TABLES = ("narrow", "rare_outside", "wide", "top_symbol")
_tables = {}


def table_and_symbols(case, nsym=70000):
    """(table, symbols, AcStat): narrow alphabet, all cached; symbols at the floor count that still occur (full-row path of
    the cached kernel); an alphabet wider than the compact rows (ac_decode_k); symbol 79 (ac_decode_k)"""
    if case not in _tables:
        rng = np.random.default_rng(1000 + TABLES.index(case))
        if case == "narrow":
            alphabet, weights = np.array([2, 11, 25, 37]), np.array([0.1, 0.2, 0.3, 0.4])
        elif case == "rare_outside":
            alphabet, weights = np.arange(20, 42), None
        elif case == "wide":
            alphabet, weights = np.arange(0, 80), None
        else:
            alphabet, weights = np.array([30, 31, 40, 78, 79]), None
        sym = rng.choice(alphabet, size=nsym, p=weights).astype(np.uint8)
        table = np.ones((6400, 80), dtype=np.uint32)
        ctxs = rng.integers(0, 6400, size=200_000)
        np.add.at(table, (ctxs, rng.choice(alphabet, size=ctxs.size, p=weights)), rng.integers(1, 50, size=ctxs.size).astype(np.uint32))
        table[:, alphabet] += 3
        if case == "rare_outside":  # 5, 70 (and 19, 42 beside the span) keep the floor count everywhere, and occur -- early too
            at = np.concatenate([np.array([2, 3, 5, 40, 63, 64, 65, 100, 101, 102]), rng.integers(103, nsym, size=nsym // 300)])
            sym[at] = rng.choice(np.array([5, 70, 19, 42], dtype=np.uint8), size=at.size)
        table = table.reshape(-1)
        _tables[case] = (table, sym, O.AcStat(table))
    return _tables[case]


def one_frame(case, n):
    """the oracle's one-frame stream of the first n symbols: [u32 size][bytes]"""
    _, sym, st = table_and_symbols(case)
    coded = st.encode_stream(sym[:n]).tobytes()
    assert len(coded) == 4 + int.from_bytes(coded[:4], "little")
    return coded


_near = {}


def sizes_near_a_reader_window(case):
    """frame sizes n whose coded size lies within 8 bytes of 256, 512 or 768 -- the bit reader takes the frame in windows of 64
    words --, one per distance found by encoding on the CPU"""
    if case not in _near:
        found = {}
        for n in range(8, 6000):
            size = len(one_frame(case, n)) - 4
            r, m = (size + 8) % 256 - 8, (size + 8) // 256
            if -8 <= r <= 8 and 1 <= m <= 3 and (m, r) not in found:
                found[(m, r)] = n
            if m > 3:
                break
        assert len(found) >= 36 and {m for m, _ in found} == {1, 2, 3}, found
        _near[case] = sorted(found.values())
    return _near[case]


SWEEP = list(range(1, 201)) + [255, 256, 257, 258, 4095, 4096, 4097, 4098, 65535, 65536, 65537]
OUT_OFFS = (0, 1, 2, 3, 5, 41, 63)
IN_OFFS = (0, 1, 3)
EVERY_ALIGNMENT = (1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 4097)


@pytest.mark.parametrize("wpb", [None, "0", "16"], ids=["wpb_default", "wpb_0", "wpb_16"])
@pytest.mark.parametrize("case", TABLES)
def test_decoder_one_frame_of_every_size_at_every_alignment(case, wpb, ctx, monkeypatch):
    """Frames of 1, 2, 3, ... symbols (the first three carry the raw symbols only), the 64-symbol flush of the output lanes at
    63..66 and 64 k +- 1, coded sizes at the edges of the bit reader's 64-word window; the output at byte offsets 0 .. 63 as
    the carry of a batch puts it, the frames at 0, 1, 3.  Every size runs at one pair of offsets, turning through all 21 pairs;
    the sizes around the lane flush run at all 21."""
    if wpb is None:
        monkeypatch.delenv("SCALCE_AC_DECODE_WPB", raising=False)
    else:
        monkeypatch.setenv("SCALCE_AC_DECODE_WPB", wpb)
    table, sym, st = table_and_symbols(case)
    dec = ctx.ac_decoder(table)
    assert dec.device_bytes > 0
    runs = [(n, OUT_OFFS[i % 7], IN_OFFS[i % 3]) for i, n in enumerate(SWEEP + sizes_near_a_reader_window(case))]
    runs += [(n, oo, io) for n in EVERY_ALIGNMENT for oo in OUT_OFFS for io in IN_OFFS]
    assert {(oo, io) for _, oo, io in runs[:len(SWEEP)]} == {(oo, io) for oo in OUT_OFFS for io in IN_OFFS}
    coded = {}
    for n, oo, io in runs:
        if n not in coded:
            coded[n] = one_frame(case, n)
        frames, out = In(coded[n], io), Out(n, oo)
        bad = dec.launch(frames.ptr, frames.nbytes, 1, n, out.ptr)
        what = f"{case} wpb {wpb}: n = {n}, out + {oo}, frames + {io}"
        assert bad == 0, what
        got = out.region(what)
        assert (got == sym[:n]).all(), f"{what}: first difference at symbol {np.flatnonzero(got != sym[:n])[:4]}"
    for n in (3, 200, 4097):  # the oracle's decoder agrees with the symbols
        assert (st.decode_block(np.frombuffer(coded[n], dtype=np.uint8)[4:], n) == sym[:n]).all()
    dec.close()


# ---- decoder: runs that start mid-stream ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_stream():
    """2 x 10 485 760 + 12 345 symbols drawn like quality strings from the narrow table: three frames, the last one short"""
    table, _, st = table_and_symbols("narrow")
    rng = np.random.default_rng(7)
    sym = rng.choice(np.array([2, 11, 25, 37]), size=2 * FRAME + 12345, p=np.array([0.1, 0.2, 0.3, 0.4])).astype(np.uint8)
    coded = st.encode_stream(sym).tobytes()
    fr = R.frames_of(coded, 3)
    assert fr[2][0] + 4 + fr[2][1] == len(coded)
    return table, sym, coded, fr


@pytest.mark.parametrize("f0,nf,exact", [(0, 3, False), (1, 2, False), (2, 1, False), (1, 1, False), (1, 1, True)],
                         ids=["all_three", "from_1", "last", "middle_rest_given", "middle_exact"])
def test_decoder_runs_from_any_frame(f0, nf, exact, ctx, long_stream, monkeypatch):
    """d_frames points at the size word of frame f0 (an odd address or not, as the sizes in front fall), nbytes is what remains
    of the stream from there or exactly the run's bytes; the output starts at an odd address and ends with nsym"""
    monkeypatch.delenv("SCALCE_AC_DECODE_WPB", raising=False)
    table, sym, coded, fr = long_stream
    dec = ctx.ac_decoder(table)
    lo = fr[f0][0]
    hi = fr[f0 + nf - 1][0] + 4 + fr[f0 + nf - 1][1] if exact else len(coded)
    want = sym[f0 * FRAME:min((f0 + nf) * FRAME, len(sym))]
    frames = In(coded[lo:hi], 1)   # the size word at an odd address
    out = Out(len(want), 41)
    # nsym outside ((nf - 1) FRAME, nf FRAME]: refused before anything is enqueued
    for nsym in ((nf - 1) * FRAME, nf * FRAME + 1):
        with pytest.raises(host.ScalceError, match=r"^\[1\]"):
            dec.launch(frames.ptr, frames.nbytes, nf, nsym, out.ptr)
    assert (out.t.cpu().numpy() == SENT).all()
    assert dec.launch(frames.ptr, frames.nbytes, nf, len(want), out.ptr) == 0
    got = out.region(f"frames {f0}..{f0 + nf - 1}")
    assert (got == want).all(), f"first difference at symbol {np.flatnonzero(got != want)[:4]} of the run"
    dec.close()


def test_decoder_short_buffer_is_a_verdict_not_a_fault(ctx, long_stream, monkeypatch):
    """The run of frames with its last 5 bytes missing -- what the CLI meets in a truncated .scalceq: the walk says so (its
    verdict word), the call returns, nothing outside the output is written"""
    monkeypatch.delenv("SCALCE_AC_DECODE_WPB", raising=False)
    table, sym, coded, fr = long_stream
    dec = ctx.ac_decoder(table)
    for f0, nf in ((2, 1), (1, 2)):
        cut = coded[fr[f0][0]:len(coded) - 5]
        frames, n = In(cut, 1), len(sym) - f0 * FRAME
        out = Out(n, 3)
        assert dec.launch(frames.ptr, frames.nbytes, nf, n, out.ptr) != 0, (f0, nf)
        got = out.region(f"short run from frame {f0}", sentinel_free=False)
        if nf == 2:  # the frame in front of the short one is whole
            assert (got[:FRAME] == sym[FRAME:2 * FRAME]).all()
    for case in TABLES:  # and one-frame streams of every kernel
        d1 = ctx.ac_decoder(table_and_symbols(case)[0])
        coded1 = one_frame(case, 4097)
        for miss in (5, len(coded1) - 3):   # inside the bytes; inside the size word
            frames, out = In(coded1[:len(coded1) - miss], 3), Out(4097, 5)
            assert d1.launch(frames.ptr, frames.nbytes, 1, 4097, out.ptr) != 0, (case, miss)
            out.region(f"{case}: short frame", sentinel_free=False)
        d1.close()
    dec.close()


# ---- records kernel -----------------------------------------------------------------------------------------------------------
# cores of one base (the shortest the table builder takes), of 12 and of 32 (the limit of a directory entry's core)
CORE12 = b"ACGTTGCAGGCT"
CORE32 = b"TTGACCAGTACGATCGGATCCATGACGTTAGC"
CORES = [b"A", b"C", b"G", b"T", CORE12, CORE32]
CORE_TEXT = b"\n".join(CORES) + b"\n"
SIZES = (20, 12, 1, 17, 20)  # buckets change at records 19 -> 20, 31 -> 32, 32 -> 33 and 49 -> 50; bucket 2 is one record
NREC = sum(SIZES)
LENGTHS = list(range(1, 41)) + [63, 64, 65, 100, 255, 256, 257, 300, 1000, 2498]


def record_set(L, seed=0):
    """70 ACGT reads of L bases in 5 buckets: core at the front (end == core length), core ending on the last base (end == L),
    one record whose core is the whole read where a core of L bases exists (else a third placement), a core that moves through
    the read record by record, the root bucket last.  Returns (reads, cores, ends)."""
    rng = np.random.default_rng(L * 7 + seed)
    ids = {c: i for i, c in enumerate(CORES)}
    front = CORE12 if L > 12 else b"A"
    last = CORE32 if L > 32 else b"G"
    whole = {1: b"T", 12: CORE12, 32: CORE32}.get(L, b"T")
    mid = CORE12 if L >= 14 else b"C"
    plan = [(front, lambda i: len(front)), (last, lambda i: L), (whole, lambda i: len(whole) + (L - len(whole)) // 3),
            (mid, lambda i: len(mid) + i % (L - len(mid) + 1)), (b"", lambda i: 0)]
    reads, cores, ends = [], [], []
    for (core, end_of), cnt in zip(plan, SIZES):
        cores.append((ids[core] if core else R.ROOT_CORE, core, cnt))
        for i in range(cnt):
            e = end_of(i)
            r = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes())
            if core:
                r[e - len(core):e] = core
            reads.append(bytes(r))
            ends.append(e)
    return reads, cores, ends


def symbols_for(n, L, seed):
    q = np.random.default_rng(seed).integers(0, 63, size=(n, L)).astype(np.uint8)  # 0 (an N) among them
    q[0, 0] = 0
    q[-1, -1] = 0
    return q


def stored_names(n, seed, longest=20):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(48, 123, size=rng.integers(0, longest + 1)).astype(np.uint8)) for _ in range(n)]


def dev_directory(directory):
    arr = (host.FqBucket * len(directory))()
    for b, e in zip(arr, directory):
        b.first, b.off, b.core_len, b.rec_bytes = e["first"], e["off"], e["core_len"], e["rec_bytes"]
        C.memmove(C.addressof(b) + host.FqBucket.core.offset, e["core"], len(e["core"]))
    return In(bytes(arr), 0, slack=0)


def run_window(ctx, L, slice_and_dir, has_buckets, n, out_ptr, first=0, d_qual=None, phred=33, names=None, library=None,
               mate_digit=0, want_offsets=False, interleave=0, pair_L=0, pair_name_off=None, reads_at=0):
    """one scalce_fastq_records_window call over buffers placed here; returns the record offsets (or None)"""
    import torch
    sl, directory = slice_and_dir
    d_reads, d_dir = In(sl, reads_at), dev_directory(directory)
    keep = [d_reads, d_dir]
    kw = {}
    if names is not None:
        payload, noff = R.pack_names(names)
        keep += [In(payload, 1), dev_u64(noff)]
        kw.update(d_names=keep[-2].ptr, d_name_off=keep[-1].data_ptr())
        if pair_name_off is not None:
            keep.append(dev_u64(pair_name_off))
            kw.update(d_pair_name_off=keep[-1].data_ptr())
    else:
        kw.update(library=library)
    roff = None
    if want_offsets:
        roff = torch.full((n + 1 + 2,), -1, dtype=torch.int64, device=DEV)  # a guard entry on both sides
        kw.update(d_record_offsets=roff.data_ptr() + 8)
    ctx.fastq_records_window(d_reads.ptr, d_dir.ptr, len(directory), L, n, out_ptr, first_record=first, has_buckets=has_buckets,
                             mate_digit=mate_digit, d_qual=d_qual, phred=phred, interleave=interleave, pair_read_len=pair_L, **kw)
    torch.cuda.synchronize()
    if roff is None:
        return None
    h = roff.cpu().numpy()
    assert h[0] == -1 and h[-1] == -1, "entries beside the record offsets were written"
    return [int(v) for v in h[1:-1]]


@pytest.mark.parametrize("has_buckets,qual,phred", [(1, True, 33), (1, True, 64), (0, True, 33), (1, False, 0), (0, False, 0)],
                         ids=["buckets_q33", "buckets_q64", "bare_q33", "buckets_two_line", "bare_two_line"])
def test_records_every_read_length_and_core_placement(has_buckets, qual, phred, ctx):
    for L in LENGTHS:
        reads, cores, ends = record_set(L)
        q = symbols_for(NREC, L, L) if qual else None
        names = stored_names(NREC, L)
        want, offs = R.text_of(reads, q, names, phred, 0)
        d_q = In(q.tobytes(), 1) if qual else None   # an odd address
        out = Out(len(want), L % 7)
        got_offs = run_window(ctx, L, R.pack_records(reads, cores if has_buckets else None, ends, L, has_buckets), has_buckets, NREC,
                              out.ptr, d_qual=d_q.ptr if qual else None, phred=phred, names=names, want_offsets=True, reads_at=L % 4)
        got = out.region(f"L = {L}").tobytes()
        assert got == want, f"L = {L}: first difference at byte {next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)}"
        assert got_offs == offs, f"L = {L}"
        assert not qual or b"N" in want


@pytest.mark.parametrize("mode", ["names", "library"])
@pytest.mark.parametrize("L", [5, 100, 257])
def test_records_windows_cut_anywhere(L, mode, ctx):
    """records [a, b) for every a and b = a + 1, 31, 32, 33 and the end: the directory starts mid-bucket, headers are inline
    in the slice, bucket changes fall on and beside a wave's 32-record edge; each window's text and offsets are the whole's"""
    reads, cores, ends = record_set(L, seed=1)
    q = symbols_for(NREC, L, 50 + L)
    names = stored_names(NREC, 60 + L) if mode == "names" else None
    base = 65  # made-up names: 65 .. 134, two and three digits
    want, offs = R.text_of(reads, q, names if names else (b"lib", base), 33, 0)
    d_q = In(q.tobytes(), 1)
    pieces = {}
    for a in range(NREC):
        for b in sorted({min(NREC, a + k) for k in (1, 31, 32, 33)} | {NREC}):
            out = Out(offs[b] - offs[a], a % 7)
            got_offs = run_window(ctx, L, R.window_records(reads, cores, ends, L, 1, a, b), 1, b - a, out.ptr, first=base + a if not names else a,
                                  d_qual=d_q.ptr + a * L, names=names[a:b] if names else None, library=None if names else b"lib",
                                  want_offsets=True, reads_at=a % 5)
            got = out.region(f"[{a}, {b})").tobytes()
            assert got == want[offs[a]:offs[b]], f"window [{a}, {b})"
            assert got_offs == [o - offs[a] for o in offs[a:b + 1]], f"window [{a}, {b})"
            pieces[(a, b)] = got
    for step in (1, 31, 32, 33):  # and end to end they are the text
        assert b"".join(pieces[(a, min(NREC, a + step))] for a in range(0, NREC, step)) == want


@pytest.mark.parametrize("mate_digit", [0, ord("1"), ord("2")])
def test_records_stored_names(mate_digit, ctx):
    """names of 0 .. 255 bytes; with a mate digit, the trailing "/x" of a name of two or more characters gets it -- "/" alone
    does not"""
    L = 9
    special = [b"/", b"/1", b"a/1", b"a/2", b"a/x", b"", b"b", b"bc", b"d" * 15, b"e" * 16, b"f" * 254, b"g" * 255, b"h" * 253 + b"/1",
               b"//", b"a/1x"]
    names = (special + stored_names(NREC, 3))[:NREC]
    reads, cores, ends = record_set(L, seed=2)
    q = symbols_for(NREC, L, 9)
    want, offs = R.text_of(reads, q, names, 33, mate_digit)
    d_q, out = In(q.tobytes(), 3), Out(len(want), 2)
    got_offs = run_window(ctx, L, R.pack_records(reads, cores, ends, L, 1), 1, NREC, out.ptr, d_qual=d_q.ptr, names=names,
                          mate_digit=mate_digit, want_offsets=True)
    assert out.region().tobytes() == want and got_offs == offs
    lines = want.split(b"\n")[0::4]
    assert lines[0] == b"@/" and lines[1] == (b"@/" + bytes([mate_digit]) if mate_digit else b"@/1") and lines[14] == b"@a/1x"


CROSSINGS = [10, 100, 10 ** 9, 2 ** 32, 10 ** 12, 10 ** 19]


@pytest.mark.parametrize("liblen", [0, 1, 255])
@pytest.mark.parametrize("qual", [True, False], ids=["fastq", "two_line"])
def test_records_made_up_names_across_digit_and_word_edges(liblen, qual, ctx):
    """"<library>.<first_record + k>": windows whose index gains a digit (9 -> 10, 99 -> 100, 10^9, 10^12), passes 2^32, and ends
    at 10^19 -- positions and digits in 64 bits; first_record is only a number, so none of this costs anything"""
    L = 36
    lib = b"Z" * liblen
    reads, cores, ends = record_set(L, seed=3)
    q = symbols_for(NREC, L, 11) if qual else None
    d_q = In(q.tobytes(), 1) if qual else None
    for edge in CROSSINGS:
        for first, n in ((edge - NREC, NREC), (edge - 35, NREC), (edge - 3, 6)) if edge < 10 ** 19 else ((edge - NREC, NREC), (edge - 2, 2)):
            if first < 0:
                continue
            a = NREC - n if edge == 10 ** 19 and n < NREC else 0
            want, offs = R.text_of(reads[a:a + n], q[a:a + n] if qual else None, (lib, first), 33, 0)
            out = Out(len(want), 5)
            got_offs = run_window(ctx, L, R.window_records(reads, cores, ends, L, 1, a, a + n), 1, n, out.ptr, first=first,
                                  d_qual=d_q.ptr + a * L if qual else None, library=lib, want_offsets=True)
            assert out.region(f"first = {first}").tobytes() == want, f"library of {liblen}, records {first} .. {first + n - 1}"
            assert got_offs == offs, f"first = {first}"


def test_records_library_of_256_characters_is_refused(ctx):
    L = 8
    reads, cores, ends = record_set(L)
    out = Out(64)
    with pytest.raises(host.ScalceError, match="library name longer than 255 characters"):
        run_window(ctx, L, R.pack_records(reads, cores, ends, L, 1), 1, NREC, out.ptr, library=b"y" * 256)
    assert (out.t.cpu().numpy() == SENT).all()


@pytest.mark.parametrize("mode", ["names", "library"])
@pytest.mark.parametrize("L1,L2", [(100, 100), (36, 151), (257, 75)])
def test_records_interleaved_windows(L1, L2, mode, ctx):
    """-i: mate 1 (buckets) and mate 2 (bare records) of a window go into ONE text by two calls, each placing its records by
    the other mate's read length and names; pair offsets and the text's end come from mate 1's call.  Windows as above."""
    reads1, cores, ends = record_set(L1, seed=4)
    reads2 = record_set(L2, seed=5)[0]
    q1, q2 = symbols_for(NREC, L1, 21), symbols_for(NREC, L2, 22)
    n1 = [x + b"/1" for x in stored_names(NREC, 23, 30)] if mode == "names" else None   # unequal lengths in the two mates
    n2 = [x + b"/7" for x in stored_names(NREC, 24, 9)] if mode == "names" else None
    base = 65 if mode == "library" else 0   # made-up names: pairs 65 .. 134, through 99 -> 100
    nm = (lambda a, b: (n1[a:b], n2[a:b])) if n1 else (lambda a, b: ((b"pe", base + a), (b"pe", base + a)))
    want, offs = R.text_of(reads1, q1, nm(0, NREC)[0], 33, ord("1"), interleave=(reads2, q2, nm(0, NREC)[1], 33, ord("2")))
    d_q1, d_q2 = In(q1.tobytes(), 1), In(q2.tobytes(), 3)
    for a in range(NREC):
        for b in sorted({min(NREC, a + k) for k in (1, 31, 32, 33)} | {NREC}):
            out = Out(offs[b] - offs[a], a % 7)
            w1, w2 = nm(a, b)
            off1 = R.pack_names(w1)[1] if n1 else None
            off2 = R.pack_names(w2)[1] if n1 else None
            got_offs = run_window(ctx, L1, R.window_records(reads1, cores, ends, L1, 1, a, b), 1, b - a, out.ptr, first=base + a,
                                  d_qual=d_q1.ptr + a * L1, names=w1 if n1 else None, library=None if n1 else b"pe", mate_digit=ord("1"),
                                  want_offsets=True, interleave=1, pair_L=L2, pair_name_off=off2)
            run_window(ctx, L2, R.window_records(reads2, None, None, L2, 0, a, b), 0, b - a, out.ptr, first=base + a,
                       d_qual=d_q2.ptr + a * L2, names=w2 if n1 else None, library=None if n1 else b"pe", mate_digit=ord("2"),
                       interleave=2, pair_L=L1, pair_name_off=off1)
            assert out.region(f"pairs [{a}, {b})").tobytes() == want[offs[a]:offs[b]], f"pairs [{a}, {b})"
            assert got_offs == [o - offs[a] for o in offs[a:b + 1]], f"pairs [{a}, {b})"
