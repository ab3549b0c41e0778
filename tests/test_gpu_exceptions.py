"""-m gpu: the letters and qualities the archive does not keep, through the C ABI (scalce_batch_set_keep_bases,
SCALCE_OUT_EXCEPTIONS, scalce_fastq_exception_window).

Count, write and gather: for crafted texts OUT_EXCEPTIONS of each mate is exception_ref's entries of the text in the order of
the batch's own OUT_PERM, scalce_batch_exceptions_info agrees, and every other output is byte for byte that of the same batch
without the option.  Then pieces cut inside the sequence and quality lines, mates, record shapes, quality maps, lean batches,
and the apply pass of the decode side on its own against exception_ref."""
import os

import numpy as np
import pytest

import exception_ref as ER
from gpu_util import device_bytes
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
STREAMS = (("reads", host.OUT_READS), ("names", host.OUT_NAMES), ("qual", host.OUT_QUAL), ("table", host.OUT_TABLE))
LOWER = np.frombuffer(b"acgtn", dtype=np.uint8)
ODD = np.frombuffer(b"RYKMSWBDHVUXryksw", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def clean(n, L, seed):
    """reads without a single exception: A C G T, no quality at the offset"""
    bases, quals = synth.reads_and_quals(n, L, seed=seed, dup_frac=0.1)
    return bases.copy(), quals.copy()


def with_pattern(n, L, seed, pattern):
    bases, quals = clean(n, L, seed)
    rng = np.random.default_rng(seed + 7)
    if pattern == "none":
        pass
    elif pattern == "first":
        bases[:, 0] |= 0x20
    elif pattern == "last":
        bases[:, L - 1] = ord("N")     # (its quality is '#' or above: an exception)
    elif pattern == "one_record":
        bases[n // 2, :] = ODD[rng.integers(0, len(ODD), L)]
    elif pattern == "every_record":
        bases[np.arange(n), rng.integers(0, L, n)] = ord("n")
    elif pattern == "random":
        hit = rng.random(bases.shape) < 0.01
        kind = rng.integers(0, 4, bases.shape)
        bases[hit & (kind == 0)] |= 0x20
        bases[hit & (kind == 1)] = ord("N")
        bases[hit & (kind == 2)] = ODD[rng.integers(0, len(ODD), int((hit & (kind == 2)).sum()))]
        quals[hit & (kind == 3)] = ord("!")
        free = rng.random(bases.shape) < 0.01          # N with the offset quality: no exception
        bases[free], quals[free] = ord("N"), ord("!")
    elif pattern == "all_lower":
        bases |= 0x20
    else:
        raise ValueError(pattern)
    return bases, quals


def text_of(bases, quals, prefix="s.", suffix="", fasta=False, lens=None):
    out = []
    for i in range(len(bases)):
        k = bases.shape[1] if lens is None else int(lens[i])
        head = (b">" if fasta else b"@") + prefix.encode() + b"%d" % i + suffix.encode() + b"\n"
        out.append(head + bases[i, :k].tobytes() + b"\n" if fasta else head + bases[i, :k].tobytes() + b"\n+\n" + quals[i, :k].tobytes() + b"\n")
    return b"".join(out)


def run(ctx, text, L, n, text2=None, L2=0, keep=True, lean=False, **kw):
    import torch
    t1 = device_bytes(text)
    t2 = device_bytes(text2) if text2 is not None else None
    b = host.Batch(ctx, L, max_reads=n + 8, max_text=max(len(text), len(text2 or b"")) + 64, paired=text2 is not None or kw.get("interleaved", False),
                   read_len2=L2, keep_bases=keep, **kw)
    if lean:
        b.set_lean(True)
    b.compress(t1.data_ptr(), len(text), t2.data_ptr() if t2 is not None else None, len(text2 or b""))
    b.finish()
    torch.cuda.synchronize()
    return b


def outputs(b, mates=1, qual=True, lengths=False):
    out = {}
    for m in range(mates):
        for key, which in STREAMS[:4 if qual else 2]:
            out[key, m] = b.output(which, 0 if which == host.OUT_NAMES else m).tobytes()
        if lengths:
            out["lengths", m] = b.output(host.OUT_LENGTHS, m).tobytes()
    out["perm"] = b.output(host.OUT_PERM, 0, np.uint32).tobytes()
    return out


def check_exceptions(b, mates, perm=None):
    """mates: per mate (bases, quals or None, offset, values, lens or None)"""
    perm = b.output(host.OUT_PERM, 0, np.uint32) if perm is None else perm
    for m, (bases, quals, off, vals, lens) in enumerate(mates):
        want = ER.entries(bases, quals, off, vals, perm=perm, lens=lens)
        got = b.output(host.OUT_EXCEPTIONS, m, np.uint64)
        assert len(got) == len(want) and (got == want).all(), f"mate {m + 1}"
        assert b.exceptions_info(m) == (len(want), ER.records_with_one(bases, quals, off, vals, lens)), f"mate {m + 1}"


def check_against_plain(ctx, bases, quals, **kw):
    n, L = bases.shape
    text = text_of(bases, quals)
    bk = run(ctx, text, L, n, **kw)
    bp = run(ctx, text, L, n, keep=False, **kw)
    check_exceptions(bk, [(bases, quals, 33, ER.IDENTITY, None)])
    assert outputs(bk) == outputs(bp)
    assert bp.output_ptr(host.OUT_EXCEPTIONS, 0)[1] == 0 and bp.exceptions_info(0) == (0, 0)   # nothing without the option
    return bk


# ---- count, write and gather ------------------------------------------------------------------------------------------------
SHAPES = [(257, L) for L in (1, 3, 4, 15, 16, 17, 63, 64, 65, 100, 255, 300)] + [(n, 100) for n in (1, 2, 1300)]


@pytest.mark.parametrize("n,L", SHAPES)
def test_random_exceptions_in_archive_order(n, L, ctx):
    """L = 15 .. 17, 63 .. 65: around the 16 bytes of a lane's step; 100, 255, 300: one, two and three steps of a row's eight
    lanes; 257 and 1300 records: more than one workgroup of 32 rows"""
    bases, quals = with_pattern(n, L, 100 + n + L, "random")
    check_against_plain(ctx, bases, quals)


PATTERNS = [(n, L, p) for n, L in ((257, 100), (257, 17), (257, 300)) for p in ("none", "first", "last", "one_record", "every_record")]
PATTERNS.append((300, 100, "all_lower"))   # 30 000 entries: the store crosses several workgroups' rows


@pytest.mark.parametrize("n,L,pattern", PATTERNS)
def test_exception_patterns(n, L, pattern, ctx):
    bases, quals = with_pattern(n, L, 200 + n + L, pattern)
    b = check_against_plain(ctx, bases, quals)
    x, rows = b.exceptions_info(0)
    want = {"none": (0, 0), "first": (n, n), "last": (n, n), "one_record": (L, 1), "every_record": (n, n), "all_lower": (n * L, n)}[pattern]
    assert (x, rows) == want


def test_two_runs_of_one_input_give_the_same_bytes(ctx):
    bases, quals = with_pattern(1300, 100, 31, "random")
    text = text_of(bases, quals)
    a = run(ctx, text, 100, 1300).output(host.OUT_EXCEPTIONS, 0).tobytes()
    assert a == run(ctx, text, 100, 1300).output(host.OUT_EXCEPTIONS, 0).tobytes() and len(a) > 8 * 1000   # (1 % of 130 000 positions)


# ---- pieces -------------------------------------------------------------------------------------------------------------------
def run_pieces(ctx, text, L, cuts, nrec):
    """the text through scalce_batch_append in pieces that end at `cuts` (what a piece leaves over opens the next one)"""
    b = host.Batch(ctx, L, max_reads=nrec + 8, max_text=len(text) + 64, keep_bases=True)
    at = 0
    for i, end in enumerate(list(cuts) + [len(text)]):
        final = i == len(cuts)
        piece = text[at:end]
        t = device_bytes(piece) if piece else None
        used, _ = b.append(t.data_ptr() if piece else None, len(piece), final=final)
        assert not final or used == len(piece)
        at += used
    b.order(); b.emit(); b.entropy(); b.finish()
    return b


def test_appended_pieces_cut_inside_the_sequence_and_quality_lines(ctx):
    n, L = 40, 20
    bases, quals = with_pattern(n, L, 41, "random")
    bases[17, :] = LOWER[np.arange(L) % 5]          # the record that is cut: an exception at every position
    text = text_of(bases, quals)
    whole = run(ctx, text, L, n)
    want, want_x = outputs(whole), whole.output(host.OUT_EXCEPTIONS, 0).tobytes()
    check_exceptions(whole, [(bases, quals, 33, ER.IDENTITY, None)])
    recs = text.split(b"\n")
    start = len(b"\n".join(recs[:4 * 17])) + 1
    head = len(recs[4 * 17]) + 1
    for c in range(head, head + 2 * L + 5):         # every byte of the sequence line, the '+' line and the quality line
        b = run_pieces(ctx, text, L, [start + c], n)
        assert b.output(host.OUT_EXCEPTIONS, 0).tobytes() == want_x, f"cut {c}"
        assert outputs(b) == want, f"cut {c}"
    third = len(text) // 3
    b = run_pieces(ctx, text, L, [third, 2 * third + 5], n)
    assert b.output(host.OUT_EXCEPTIONS, 0).tobytes() == want_x and outputs(b) == want


# ---- mates --------------------------------------------------------------------------------------------------------------------
def test_mates_keep_their_own_entries_and_interleaved_text_gives_the_same(ctx):
    n, L1, L2 = 400, 100, 75
    b1, q1 = with_pattern(n, L1, 51, "random")
    b2, q2 = with_pattern(n, L2, 52, "random")
    b2[n - 1, L2 - 1] = ord("n")
    t1, t2 = text_of(b1, q1, "p.", "/1"), text_of(b2, q2, "p.", "/2")
    mates = [(b1, q1, 33, ER.IDENTITY, None), (b2, q2, 33, ER.IDENTITY, None)]
    bk = run(ctx, t1, L1, n, t2, L2)
    check_exceptions(bk, mates)
    assert outputs(bk, 2) == outputs(run(ctx, t1, L1, n, t2, L2, keep=False), 2)
    two = [bk.output(host.OUT_EXCEPTIONS, m).tobytes() for m in range(2)]
    assert two[0] != two[1]
    r1, r2 = t1.split(b"\n"), t2.split(b"\n")
    il = b"".join(b"\n".join(r1[4 * k:4 * k + 4]) + b"\n" + b"\n".join(r2[4 * k:4 * k + 4]) + b"\n" for k in range(n))
    bi = run(ctx, il, L1, n, L2=L2, interleaved=True)
    check_exceptions(bi, mates)
    assert [bi.output(host.OUT_EXCEPTIONS, m).tobytes() for m in range(2)] == two
    assert outputs(bi, 2) == outputs(bk, 2)


# ---- record shapes and quality maps -------------------------------------------------------------------------------------------
def test_fasta_records(ctx):
    n, L = 500, 100
    bases, _ = with_pattern(n, L, 61, "random")
    text = text_of(bases, None, fasta=True)
    bk = run(ctx, text, L, n, fasta=True)
    check_exceptions(bk, [(bases, None, 33, ER.IDENTITY, None)])
    e = bk.output(host.OUT_EXCEPTIONS, 0, np.uint64)
    assert ((e >> np.uint64(8)) & np.uint64(255) == 0).all() and (e & np.uint64(255) == ord("N")).any()   # quality byte 0; N is one
    assert outputs(bk, qual=False) == outputs(run(ctx, text, L, n, fasta=True, keep=False), qual=False)


def test_records_whose_qualities_are_dropped(ctx):
    n, L = 500, 100
    bases, quals = with_pattern(n, L, 62, "random")
    text = text_of(bases, quals)
    bk = run(ctx, text, L, n, no_qualities=True)
    check_exceptions(bk, [(bases, None, 33, ER.IDENTITY, None)])
    assert outputs(bk, qual=False) == outputs(run(ctx, text, L, n, no_qualities=True, keep=False), qual=False)


def test_a_lossy_map_that_merges_qualities_into_the_offset(ctx):
    n, L = 500, 100
    bases, quals = with_pattern(n, L, 63, "random")
    vals = np.arange(128, dtype=np.int32)
    vals[33:50] = 33          # '!' .. '1' become '!': every base of quality 16 or less comes back as N
    vals[50:56] = 52
    assert ((quals > 33) & (quals < 50)).sum() > 100
    text = text_of(bases, quals)
    bk = run(ctx, text, L, n, qmap=[(33, vals)])
    check_exceptions(bk, [(bases, quals, 33, vals, None)])
    assert outputs(bk) == outputs(run(ctx, text, L, n, qmap=[(33, vals)], keep=False))
    assert bk.exceptions_info(0)[0] > ER.exception_mask(bases, quals).sum() + 100


def test_phred64(ctx):
    n, L = 500, 100
    bases, quals = with_pattern(n, L, 64, "random")
    quals = (quals + 31).astype(np.uint8)          # '!' -> '@'
    text = text_of(bases, quals)
    vals = np.arange(128, dtype=np.int32)
    bk = run(ctx, text, L, n, qmap=[(64, vals)])
    check_exceptions(bk, [(bases, quals, 64, ER.IDENTITY, None)])
    assert outputs(bk) == outputs(run(ctx, text, L, n, qmap=[(64, vals)], keep=False))


def test_variable_length_reads(ctx):
    n, L = 500, 100
    rng = np.random.default_rng(65)
    lens = rng.permutation(np.concatenate([np.arange(L + 1), rng.integers(0, L + 1, size=n - L - 1)]))
    bases, quals = with_pattern(n, L, 66, "random")
    has = lens > 0
    bases[np.flatnonzero(has), lens[has] - 1] = ord("n")      # an exception at each read's last real position
    text = text_of(bases, quals, lens=lens)
    bk = run(ctx, text, L, n, variable_length=True)
    # the ingest reads the padded text: N with the offset quality behind a read's end, never an exception
    pb, pq = bases.copy(), quals.copy()
    pad = np.arange(L)[None, :] >= lens[:, None]
    pb[pad], pq[pad] = ord("N"), ord("!")
    check_exceptions(bk, [(pb, pq, 33, ER.IDENTITY, None)])
    check_exceptions(bk, [(bases, quals, 33, ER.IDENTITY, lens)])
    assert outputs(bk, lengths=True) == outputs(run(ctx, text, L, n, variable_length=True, keep=False), lengths=True)


# ---- lean, refusals -------------------------------------------------------------------------------------------------------------
def test_the_stream_outlives_the_lean_releases(ctx):
    n, L = 700, 100
    bases, quals = with_pattern(n, L, 71, "random")
    text = text_of(bases, quals)
    perm = run(ctx, text, L, n, keep=False).output(host.OUT_PERM, 0, np.uint32)
    b = run(ctx, text, L, n, lean=True)
    check_exceptions(b, [(bases, quals, 33, ER.IDENTITY, None)], perm=perm)


def test_the_option_is_set_before_the_first_ingest(ctx):
    bases, quals = with_pattern(40, 50, 72, "random")
    text = text_of(bases, quals)
    t = device_bytes(text)
    b = host.Batch(ctx, 50, max_reads=64, max_text=len(text) + 64)
    b.ingest(0, t.data_ptr(), len(text))
    with pytest.raises(host.ScalceError) as e:
        b.set_keep_bases(True)
    assert "[1]" in str(e.value)


def test_sharded_runs_and_pipelines_refuse_the_batch(ctx):
    from scalce_amd.pipeline import ShardPipeline
    bases, quals = with_pattern(40, 50, 73, "random")
    text = text_of(bases, quals)
    t = device_bytes(text)
    b = host.Batch(ctx, 50, max_reads=64, max_text=len(text) + 64, bucket_set_size=1 << 20, keep_bases=True)
    comm = host.Comm(0, 1, 0, shm_name="/scalce_exceptions_%d" % os.getpid(), slot_bytes=1 << 20)
    try:
        with pytest.raises(host.ScalceError) as e:
            host.sharded_compress(comm, ctx, b, t.data_ptr(), len(text))
        assert "[1]" in str(e.value) and "--keep-bases" in str(e.value)
    finally:
        comm.close()
    with pytest.raises(RuntimeError) as e:
        ShardPipeline([b, host.Batch(ctx, 50, max_reads=64, max_text=4096)])
    assert "--keep-bases" in str(e.value)
    b.ingest(0, t.data_ptr(), len(text))
    with pytest.raises(host.ScalceError):
        b.text_offset(0, 3)


# ---- the apply pass alone -----------------------------------------------------------------------------------------------------
def window_records(n, L, qual, names, seed):
    """what fastq_records_k leaves for a window: "@name\\n" bases ["\\n+\\n" qualities] "\\n" per record"""
    bases, quals = clean(n, L, seed)
    if qual:
        return [b"@" + names[i] + b"\n" + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i in range(n)]
    return [b"@" + names[i] + b"\n" + bases[i].tobytes() + b"\n" for i in range(n)]


def apply_on_device(ctx, recs, L, qual, first, ents):
    import torch
    text = b"".join(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    d_text = device_bytes(text + bytes(64))
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    e = np.asarray(ents, dtype=np.uint64)
    d_ent = torch.from_numpy(np.concatenate([e, np.zeros(2, dtype=np.uint64)]).view(np.int64)).to("cuda:0")
    d_bad = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    host.fastq_exception_window(ctx, L, qual, first, len(recs), d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(e), d_bad.data_ptr())
    torch.cuda.synchronize()
    got = d_text.cpu().numpy().tobytes()
    assert got[len(text):] == bytes(64)
    return got[:len(text)], int(d_bad.cpu()[0])


def name_kind(kind, r, first):
    if kind == "long":
        return (b"%d" % r + b"x" * 255)[:(0, 1, 255)[r % 3]]
    return b"lib.%d" % (first + r)          # -n library names: the digit count changes inside the window


def window_entries(n, L, qual, first, rng):
    """entries in the first and the last record and at positions 0 and L - 1, and a few more"""
    picks = {(0, 0), (0, L - 1), (n - 1, 0), (n - 1, L - 1)}
    for _ in range(min(3 * n, 40)):
        picks.add((int(rng.integers(0, n)), int(rng.integers(0, L))))
    return [host.exception_entry(first + r, p, int(LOWER[(r + p) % 5]), int(35 + (r + p) % 40) if qual else 0) for r, p in sorted(picks)]


@pytest.mark.parametrize("kind,first", [("long", 0), ("long", 1000), ("library", 9), ("library", 10)])
@pytest.mark.parametrize("qual", [True, False], ids=["qualities", "two_lines"])
@pytest.mark.parametrize("n,L", [(1, 100), (2, 100), (257, 100), (257, 1)])
def test_apply_pass_against_the_reference(n, L, qual, kind, first, ctx):
    rng = np.random.default_rng(n + L + first)
    recs = window_records(n, L, qual, [name_kind(kind, r, first) for r in range(n)], 80 + n)
    ents = window_entries(n, L, qual, first, rng)
    got, bad = apply_on_device(ctx, recs, L, qual, first, ents)
    assert bad == 0
    assert got == b"".join(ER.apply_text(recs, ents, L, qual, first=first))
    assert got != b"".join(recs)
    got, bad = apply_on_device(ctx, recs, L, qual, first, [])        # zero entries: nothing is touched, the flag is cleared
    assert bad == 0 and got == b"".join(recs)


def test_apply_pass_on_an_interleaved_window(ctx):
    import torch
    n, L1, L2, first = 130, 100, 75, 40
    rng = np.random.default_rng(91)
    r1 = window_records(n, L1, True, [b"p.%d/1" % (first + r) for r in range(n)], 92)
    r2 = window_records(n, L2, True, [(b"q.%d" % r + b"y" * 40)[:1 + r % 40] for r in range(n)], 93)
    e1, e2 = window_entries(n, L1, True, first, rng), window_entries(n, L2, True, first, rng)
    recs = [x for pair in zip(r1, r2) for x in pair]
    text = b"".join(recs)
    pair_off = np.cumsum([0] + [len(a) + len(b) for a, b in zip(r1, r2)]).astype(np.uint64)
    name_off2 = np.cumsum([0] + [len(r.split(b"\n")[0]) for r in r2]).astype(np.uint64)   # a length byte and the name: '@' and the name
    d_text = device_bytes(text + bytes(64))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")  # noqa: E731
    d_pair, d_noff = dev(pair_off), dev(name_off2)
    d_e = [dev(np.asarray(e + [0], dtype=np.uint64)) for e in (e1, e2)]
    d_bad = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    d_ws = torch.zeros(host.fastq_exception_pairs_ws_bytes(n), dtype=torch.uint8, device="cuda:0")
    host.fastq_exception_window_pairs(ctx, (L1, L2), True, first, n, d_text.data_ptr(), d_pair.data_ptr(), d_noff.data_ptr(),
                                      [d.data_ptr() for d in d_e], [len(e1), len(e2)], d_bad.data_ptr(), d_ws.data_ptr())
    torch.cuda.synchronize()
    want = ER.apply_text(ER.apply_text(recs, e1, L1, True, first=first, stride=2, which=0), e2, L2, True, first=first, stride=2, which=1)
    assert int(d_bad.cpu()[0]) == 0
    assert d_text.cpu().numpy().tobytes() == b"".join(want) + bytes(64)


@pytest.mark.parametrize("qual", [True, False], ids=["qualities", "two_lines"])
def test_apply_pass_reports_an_entry_outside_its_window_or_record(qual, ctx):
    n, L, first = 5, 50, 20
    recs = window_records(n, L, qual, [b"r%d" % r for r in range(n)], 95)
    text = b"".join(recs)
    for e in (host.exception_entry(first, L, ord("n"), 40), host.exception_entry(first + n, 0, ord("n"), 40),
              host.exception_entry(first - 1, 0, ord("n"), 40), host.exception_entry(first + 4, 4095, ord("n"), 40)):
        got, bad = apply_on_device(ctx, recs, L, qual, first, [e])
        assert bad == 1 and got == text, hex(e)
