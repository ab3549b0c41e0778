"""-m gpu: what follows the names through the C ABI (scalce_batch_set_keep_comments, SCALCE_OUT_COMMENTS).

Extraction and gather: for crafted texts OUT_COMMENTS of each mate is comment_ref's entries of the text in the order of the
batch's own OUT_PERM, scalce_batch_comments_info agrees, and every other output is byte for byte that of the same batch
without the option.  Then pieces cut inside a header line, mates, record shapes, errors, lean batches, and the insert pass
of the decode side (scalce_fastq_comment_window) on its own against comment_ref."""
import os

import numpy as np
import pytest

import comment_ref as CR
from gpu_util import device_bytes, hip_compress
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
STREAMS = (("reads", host.OUT_READS), ("names", host.OUT_NAMES), ("qual", host.OUT_QUAL), ("table", host.OUT_TABLE))
# what an entry may hold behind its first space: anything but a newline (spaces and tabs included)
ALPHABET = np.frombuffer(b"ACGTN0123456789:=_/ \tabcxyz+@", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def entry(k, rng):
    return b"" if k == 0 else b" " + ALPHABET[rng.integers(0, len(ALPHABET), size=k - 1)].tobytes()


def name(k, r):
    """k characters that hold no space, different from record to record where k allows"""
    return (b"%d" % r + b"r" * k)[:k] if k else b""


def make_text(L, names, ents, seed, fasta=False, lens=None, qshift=0):
    n = len(names)
    bases, quals = synth.reads_and_quals(n, max(L, 1), seed=seed, n_frac=0.01, dup_frac=0.1)
    out = []
    for i in range(n):
        k = L if lens is None else int(lens[i])
        b, q = bases[i, :k].tobytes(), (quals[i, :k] + qshift).astype(np.uint8).tobytes()
        head = (b">" if fasta else b"@") + names[i] + ents[i]
        out.append(head + b"\n" + b + b"\n" if fasta else head + b"\n" + b + b"\n+\n" + q + b"\n")
    return b"".join(out)


def crafted(n, L, seed, **kw):
    """record r: an entry of r % 41 bytes behind a name of r % 17 characters -- every entry length from 0 to 40 meets every
    16-byte phase of source and destination"""
    rng = np.random.default_rng(seed)
    names = [name(r % 17, r) for r in range(n)]
    ents = [entry(r % 41, rng) for r in range(n)]
    return make_text(L, names, ents, seed, **kw), ents


def outputs(b, mates=1, lengths=False):
    out = {}
    for m in range(mates):
        for key, which in STREAMS:
            out[key, m] = b.output(which, 0 if which == host.OUT_NAMES else m).tobytes()
        if lengths:
            out["lengths", m] = b.output(host.OUT_LENGTHS, m).tobytes()
    out["perm"] = b.output(host.OUT_PERM, 0, np.uint32).tobytes()
    return out


def check_comments(b, ents_per_mate):
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    for m, ents in enumerate(ents_per_mate):
        want = CR.body(ents, perm)
        got = b.output(host.OUT_COMMENTS, m).tobytes()
        assert got == want, f"mate {m + 1}"
        assert b.comments_info(m) == (len(want), max((len(e) for e in ents), default=0)), f"mate {m + 1}"


def check_against_plain(ctx, text, L, ents_per_mate, text2=None, L2=0, lengths=False, **kw):
    mates = len(ents_per_mate)
    bc = hip_compress(ctx, text, L, text2, L2, keep_comments=True, **kw)
    bp = hip_compress(ctx, text, L, text2, L2, **kw)
    check_comments(bc, ents_per_mate)
    assert outputs(bc, mates, lengths) == outputs(bp, mates, lengths)
    assert bp.output_ptr(host.OUT_COMMENTS, 0)[1] == 0 and bp.comments_info(0) == (0, 0)   # nothing without the option
    return bc


# ---- extraction and gather ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(1, 100), (2, 100), (257, 100), (1300, 100), (1300, 16), (1300, 37), (1300, 300)])
def test_crafted_entries_in_archive_order(n, L, ctx):
    """257 records: the store (5.4 KB) crosses one 4 KiB span of the copy kernel's workgroup; 1300: six of them.  L = 16 and
    100 take the one-pass ingest, 37 too (no multiple of 4), 300 the indexed one."""
    text, ents = crafted(n, L, 100 + n + L)
    if n == 1300:
        assert {len(e) for e in ents} == set(range(41)) and sum(len(e) + 1 for e in ents) > 6 * 4096
    check_against_plain(ctx, text, L, [ents])


def test_names_of_0_1_15_16_and_255_characters(ctx):
    n = 300
    rng = np.random.default_rng(7)
    widths = [(0, 1, 15, 16, 255)[r % 5] for r in range(n)]
    names = [name(w, r) for r, w in enumerate(widths)]
    ents = [entry((r // 5) % 41, rng) for r in range(n)]
    check_against_plain(ctx, make_text(100, names, ents, 8), 100, [ents])


def test_hand_written_header_lines(ctx):
    """no space, space only, two spaces in a row, a space in front of the name, a tab in the name"""
    heads = [(b"r1", b""), (b"r2", b" "), (b"r3", b"  x"), (b"", b" r4 x"), (b"r\t5", b" 2:N:0"), (b"r\t6", b""),
             (b"M01:23:000-A1:1:1101:1:2", b" 1:N:0:ATCACG"), (b"SRR1.1", b" HWI-ST:1:1 length=100")]
    names, ents = [h for h, _ in heads], [e for _, e in heads]
    text = make_text(50, names, ents, 9)
    assert CR.entries(text) == [ents]
    check_against_plain(ctx, text, 50, [ents])


# ---- pieces -------------------------------------------------------------------------------------------------------------------
def run_pieces(ctx, text, L, cuts, nrec):
    """the text through scalce_batch_append in pieces that end at `cuts` (what a piece leaves over opens the next one)"""
    b = host.Batch(ctx, L, max_reads=nrec + 8, max_text=len(text) + 64, keep_comments=True)
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


def test_appended_pieces_cut_inside_a_header_line(ctx):
    n, L = 60, 50
    text, ents = crafted(n, L, 21)
    want = outputs(hip_compress(ctx, text, L))
    recs = [text[i:j] for i, j in zip(*record_bounds(text, 4))]
    assert b"".join(recs) == text and len(recs) == n
    k = 38   # name of 4 characters, entry of 38 bytes
    start = sum(len(r) for r in recs[:k])
    head = recs[k].split(b"\n")[0]
    assert len(CR.entry_of(head)) == 38 and len(head) == 1 + 4 + 38
    # every byte of the header line: in front of '@', inside the name, between the name and the space, inside the entry, in
    # front of the newline and behind it
    for c in range(len(head) + 2):
        b = run_pieces(ctx, text, L, [start + c], n)
        check_comments(b, [ents])
        assert outputs(b) == want, f"cut {c}"
    third = len(text) // 3
    b = run_pieces(ctx, text, L, [third, 2 * third + 5], n)
    check_comments(b, [ents])
    assert outputs(b) == want, "three pieces"


# ---- mates --------------------------------------------------------------------------------------------------------------------
def test_mates_keep_their_own_entries_and_interleaved_text_gives_the_same(ctx):
    n, L1, L2 = 400, 100, 75
    rng = np.random.default_rng(31)
    names = [b"p.%d" % r for r in range(n)]
    e1 = [entry(r % 41, rng) for r in range(n)]
    e2 = [entry((r * 7 + 3) % 41, rng) for r in range(n)]
    t1 = make_text(L1, [x + b"/1" for x in names], e1, 32)
    t2 = make_text(L2, [x + b"/2" for x in names], e2, 33)
    bp = check_against_plain(ctx, t1, L1, [e1, e2], t2, L2)
    two = [bp.output(host.OUT_COMMENTS, m).tobytes() for m in range(2)]
    assert two[0] != two[1]
    r1, r2 = t1.split(b"\n"), t2.split(b"\n")
    il = b"".join(b"\n".join(r1[4 * k:4 * k + 4]) + b"\n" + b"\n".join(r2[4 * k:4 * k + 4]) + b"\n" for k in range(n))
    assert CR.entries(il, interleaved=True) == [e1, e2]
    t = device_bytes(il)
    bi = host.Batch(ctx, L1, max_reads=n + 8, max_text=len(il) + 64, paired=True, read_len2=L2, interleaved=True, keep_comments=True)
    bi.compress(t.data_ptr(), len(il))
    bi.finish()
    check_comments(bi, [e1, e2])
    assert [bi.output(host.OUT_COMMENTS, m).tobytes() for m in range(2)] == two
    assert outputs(bi, 2) == outputs(bp, 2)


# ---- record shapes ------------------------------------------------------------------------------------------------------------
def test_fasta_records(ctx):
    text, ents = crafted(500, 100, 41, fasta=True)
    assert CR.entries(text, lines_per_record=2) == [ents]
    tc = device_bytes(text)
    out = []
    for keep in (True, False):
        b = host.Batch(ctx, 100, max_reads=508, max_text=len(text) + 64, fasta=True, keep_comments=keep)
        b.compress(tc.data_ptr(), len(text))
        b.finish()
        out.append({k: b.output(w, 0).tobytes() for k, w in STREAMS[:2]})
        out[-1]["perm"] = b.output(host.OUT_PERM, 0, np.uint32).tobytes()
        if keep:
            check_comments(b, [ents])
    assert out[0] == out[1]


def test_records_whose_qualities_are_dropped(ctx):
    text, ents = crafted(500, 100, 42)
    check_against_plain(ctx, text, 100, [ents], no_qualities=True)


def test_variable_length_reads(ctx):
    n, L = 500, 100
    rng = np.random.default_rng(43)
    lens = rng.permutation(np.concatenate([np.arange(L + 1), rng.integers(0, L + 1, size=n - L - 1)]))
    names = [b"v.%d" % r for r in range(n)]
    ents = [entry(r % 41, rng) for r in range(n)]
    text = make_text(L, names, ents, 44, lens=lens)
    check_against_plain(ctx, text, L, [ents], lengths=True, variable_length=True)


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_an_entry_of_65535_bytes_is_kept_and_one_more_is_an_error(ctx):
    rng = np.random.default_rng(51)
    names = [b"a", b"b", b"c"]
    ents = [b" x", entry(65535, rng), b""]
    b = check_against_plain(ctx, make_text(50, names, ents, 52), 50, [ents])
    assert b.comments_info(0)[1] == 65535
    ents[1] = entry(65536, rng)
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, make_text(50, names, ents, 52), 50, keep_comments=True)
    assert "[3]" in str(e.value) and "(ERROR) record 1: what follows the name is longer than 65535 bytes" in str(e.value)
    hip_compress(ctx, make_text(50, names, ents, 52), 50)   # without the option the text is the archive it was


def test_the_setter_refuses_a_batch_without_names(ctx):
    b = host.Batch(ctx, 50, max_reads=64, max_text=4096, use_names=False)
    with pytest.raises(host.ScalceError) as e:
        b.set_keep_comments(True)
    assert "[1]" in str(e.value)
    b.set_keep_comments(False)
    with pytest.raises(host.ScalceError):
        host.Batch(ctx, 50, max_reads=64, max_text=4096, use_names=False, keep_comments=True)


def test_sharded_runs_and_pipelines_refuse_the_batch(ctx):
    from scalce_amd.pipeline import ShardPipeline
    text, _ = crafted(40, 50, 61)
    t = device_bytes(text)
    b = host.Batch(ctx, 50, max_reads=64, max_text=len(text) + 64, bucket_set_size=1 << 20, keep_comments=True)
    comm = host.Comm(0, 1, 0, shm_name="/scalce_comments_%d" % os.getpid(), slot_bytes=1 << 20)
    try:
        with pytest.raises(host.ScalceError) as e:
            host.sharded_compress(comm, ctx, b, t.data_ptr(), len(text))
        assert "[1]" in str(e.value) and "--keep-comments" in str(e.value)
    finally:
        comm.close()
    with pytest.raises(RuntimeError) as e:
        ShardPipeline([b, host.Batch(ctx, 50, max_reads=64, max_text=4096)])
    assert "--keep-comments" in str(e.value)
    b.ingest(0, t.data_ptr(), len(text))
    with pytest.raises(host.ScalceError):
        b.text_offset(0, 3)


# ---- lean ---------------------------------------------------------------------------------------------------------------------
def test_the_stream_outlives_the_lean_releases(ctx):
    n, L = 700, 100
    text, ents = crafted(n, L, 71)
    perm = hip_compress(ctx, text, L).output(host.OUT_PERM, 0, np.uint32)
    t = device_bytes(text)
    b = host.Batch(ctx, L, max_reads=n + 8, max_text=len(text) + 64, keep_comments=True)
    b.set_lean(True)
    b.compress(t.data_ptr(), len(text))
    b.finish()
    want = CR.body(ents, perm)
    assert b.output(host.OUT_COMMENTS, 0).tobytes() == want
    assert b.comments_info(0) == (len(want), 40)


# ---- the insert pass alone ----------------------------------------------------------------------------------------------------
def window_text(n, L, qual, made_up, seed):
    """what fastq_records_k leaves for a window: "@name\\n" bases ["\\n+\\n" qualities] "\\n" per record"""
    names = [b"lib.%d" % (1000 + r) if made_up else name(1 + r % 40, r) for r in range(n)]
    text = make_text(L, names, [b""] * n, seed)
    recs = [text[i:j] for i, j in zip(*record_bounds(text, 4))]
    if not qual:
        recs = [r.split(b"\n")[0] + b"\n" + r.split(b"\n")[1] + b"\n" for r in recs]
    return recs


def record_bounds(text, lpr):
    ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)[lpr - 1::lpr] + 1
    return np.concatenate([[0], ends[:-1]]), ends


@pytest.mark.parametrize("kind", ["empty", "longest", "mixed"])
@pytest.mark.parametrize("made_up", [False, True], ids=["stored", "made_up"])
@pytest.mark.parametrize("qual", [True, False], ids=["qualities", "two_lines"])
@pytest.mark.parametrize("n,L", [(1, 100), (2, 100), (257, 100), (257, 300)])
def test_insert_pass_against_the_reference(n, L, qual, made_up, kind, ctx):
    import torch
    rng = np.random.default_rng(n + L)
    C = 40
    ents = [b"" if kind == "empty" else entry(C if kind == "longest" else r % (C + 1), rng) for r in range(n)]
    recs = window_text(n, L, qual, made_up, 80 + n)
    text = b"".join(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    body = CR.body(ents)
    want, want_off = CR.insert(text, off, ents, lines_per_record=4 if qual else 2)
    d_text, d_ent = device_bytes(text), device_bytes(body)
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    d_out = torch.zeros(len(text) + len(body) + 64, dtype=torch.uint8, device="cuda:0")
    d_out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    d_bad = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    d_ws = torch.zeros(host.fastq_comment_ws_bytes(n, len(body)), dtype=torch.uint8, device="cuda:0")
    host.fastq_comment_window(ctx, L, qual, n, d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(body), d_out.data_ptr(),
                              d_out_off.data_ptr(), d_bad.data_ptr(), d_ws.data_ptr())
    torch.cuda.synchronize()
    assert int(d_bad.cpu()[0]) == 0
    assert (d_out_off.cpu().numpy().view(np.uint64) == want_off).all()
    got = d_out.cpu().numpy().tobytes()
    assert got[:len(want)] == want and got[len(want):] == bytes(len(got) - len(want))   # nothing behind the text's end


def test_insert_pass_reports_entries_that_do_not_fit_the_records(ctx):
    import torch
    n, L = 5, 50
    recs = window_text(n, L, True, False, 90)
    text = b"".join(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    d_text = device_bytes(text)
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    for body in (b" a\n b\n c\n d\n", b" a\n b\n c\n d\n e\n f\n", b" a\n b\n c\n d\n e"):
        d_ent = device_bytes(body)
        d_out = torch.zeros(len(text) + len(body) + 64, dtype=torch.uint8, device="cuda:0")
        d_out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        d_ws = torch.zeros(host.fastq_comment_ws_bytes(n, len(body)), dtype=torch.uint8, device="cuda:0")
        host.fastq_comment_window(ctx, L, True, n, d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(body), d_out.data_ptr(),
                                  d_out_off.data_ptr(), d_bad.data_ptr(), d_ws.data_ptr())
        torch.cuda.synchronize()
        assert int(d_bad.cpu()[0]) == 1, body
