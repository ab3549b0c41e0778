"""-m gpu: the '+' lines through the C ABI (scalce_batch_set_keep_plus, SCALCE_OUT_PLUS, scalce_fastq_plus_window).

Compress: for crafted texts OUT_PLUS of each mate is plus_ref's entries of the text in the order of the batch's own OUT_PERM,
scalce_batch_plus_info agrees, and every other output is byte for byte that of the same batch without the option.  Then the
two errors of the option, pieces cut at every byte, interleaved text, an all-bare input, refusals.  Insert: the pass of the
decode side on its own against plus_ref, for windows as fastq_records_k, the comment insert and the strip leave them."""
import os

import numpy as np
import pytest

import comment_ref as CR
import plus_ref as PR
from gpu_util import device_bytes, hip_compress
from scalce_amd import format as fmt
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
STREAMS = (("reads", host.OUT_READS), ("names", host.OUT_NAMES), ("qual", host.OUT_QUAL), ("table", host.OUT_TABLE))
ALPHABET = np.frombuffer(b"ACGTN0123456789:=_/ \tabcxyz+@'", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def header(h, r, rng):
    """a header line of h bytes: '@', a name without a space, and -- from 8 bytes on -- a comment behind a space"""
    if h < 8:
        return (b"@" + b"%d" % r + b"n" * h)[:h]
    k = 2 + r % (h - 5)
    return (b"@" + (b"%d" % r + b"n" * h)[:k] + b" " + ALPHABET[rng.integers(0, len(ALPHABET), size=h)].tobytes())[:h]


def third(kind, head, r, rng):
    if kind == 0:
        return b"+"
    if kind == 1:
        return b"+" + head[1:]
    if kind == 2:                                   # the header line with another last byte
        return b"+" + head[1:-1] + (b"#" if head[-1:] != b"#" else b"$") if len(head) > 1 else b"+#"
    if kind == 3:                                   # ... one byte shorter
        return b"+" + head[1:-1] if len(head) > 2 else b"+="
    if kind == 4:                                   # ... one byte longer
        return b"+" + head[1:] + b"x"
    if kind == 5:                                   # literals that begin with the class bytes
        return (b"+=", b"+'", b"+=" + head[1:], b"+'" + head[1:])[r % 4]
    return b"+" + ALPHABET[rng.integers(0, len(ALPHABET), size=1 + r % 43)].tobytes()


def make_text(L, heads, thirds, seed, lens=None):
    n = len(heads)
    bases, quals = synth.reads_and_quals(n, max(L, 1), seed=seed, n_frac=0.01, dup_frac=0.1)
    out = []
    for i in range(n):
        k = L if lens is None else int(lens[i])
        out.append(heads[i] + b"\n" + bases[i, :k].tobytes() + b"\n" + thirds[i] + b"\n" + quals[i, :k].tobytes() + b"\n")
    return b"".join(out)


def crafted(n, L, seed, kinds=7, **kw):
    """record r: a header line of 1 + r % 40 bytes and a third line of kind (r // 40 + r) % kinds -- every header length meets
    every kind, and the third lines begin at every byte phase of 4 and of 16"""
    rng = np.random.default_rng(seed)
    heads = [header(1 + r % 40, r, rng) for r in range(n)]
    thirds = [third((r // 40 + r) % kinds, heads[r], r, rng) for r in range(n)]
    return make_text(L, heads, thirds, seed, **kw)


def outputs(b, mates=1, lengths=False):
    out = {}
    for m in range(mates):
        for key, which in STREAMS:
            out[key, m] = b.output(which, 0 if which == host.OUT_NAMES else m).tobytes()
        if lengths:
            out["lengths", m] = b.output(host.OUT_LENGTHS, m).tobytes()
    out["perm"] = b.output(host.OUT_PERM, 0, np.uint32).tobytes()
    return out


def check_plus(b, ents_per_mate):
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    for m, ents in enumerate(ents_per_mate):
        want = PR.body(ents, perm)
        got = b.output(host.OUT_PLUS, m).tobytes()
        assert got == want, f"mate {m + 1}"
        assert b.plus_info(m) == (len(want), max((len(e) for e in ents), default=0), sum(e == b"=" for e in ents),
                                  sum(len(e) > 1 for e in ents)), f"mate {m + 1}"


def check_against_plain(ctx, text, L, text2=None, L2=0, lengths=False, **kw):
    ents = PR.entries(text) + (PR.entries(text2) if text2 is not None else [])
    bk = hip_compress(ctx, text, L, text2, L2, keep_plus=True, **kw)
    bp = hip_compress(ctx, text, L, text2, L2, **kw)
    check_plus(bk, ents)
    assert outputs(bk, len(ents), lengths) == outputs(bp, len(ents), lengths)
    assert bp.output_ptr(host.OUT_PLUS, 0)[1] == 0 and bp.plus_info(0) == (0, 0, 0, 0)   # nothing without the option
    return bk


# ---- extraction and gather ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(1, 100), (2, 100), (281, 100), (1400, 100), (1400, 16), (1400, 37), (1400, 300)])
def test_crafted_lines_in_archive_order(n, L, ctx):
    """1400 records: the store crosses several 4 KiB spans of the extract kernel's workgroups, and every header length of 1 to
    40 bytes meets all seven kinds of third line.  L = 16, 100 and 37 take the one-pass ingest, 300 the indexed one."""
    text = crafted(n, L, 100 + n + L)
    ents = PR.entries(text)[0]
    if n == 1400:
        lines = text.split(b"\n")
        assert {e[:1] for e in ents} == {b"", b"=", b"'"} and sum(len(e) + 1 for e in ents) > 3 * 4096
        assert {len(h) for h in lines[0:-1:4]} == set(range(1, 41))
        assert {sum(len(x) + 1 for x in lines[:4 * r + 2]) % 16 for r in range(n)} == set(range(16))
    check_against_plain(ctx, text, L)


def test_a_repeat_that_differs_in_its_last_byte_or_by_one_in_length(ctx):
    heads = [b"@SRR001666.%d 071112_SLXA-EAS1_s_7:5:1:817:%d length=36" % (r, 345 + r) for r in range(8)]
    thirds = [b"+" + heads[0][1:], b"+" + heads[1][1:-1] + b"7", b"+" + heads[2][1:-1], b"+" + heads[3][1:] + b"6",
              b"+" + b"X" + heads[4][2:], b"+", b"+" + heads[6][1:5], b"+" + heads[7][1:]]
    text = make_text(36, heads, thirds, 5)
    assert [e[:1] for e in PR.entries(text)[0]] == [b"=", b"'", b"'", b"'", b"'", b"", b"'", b"="]
    check_against_plain(ctx, text, 36)


def test_variable_length_reads(ctx):
    n, L = 500, 100
    rng = np.random.default_rng(43)
    lens = rng.permutation(np.concatenate([np.arange(L + 1), rng.integers(0, L + 1, size=n - L - 1)]))
    check_against_plain(ctx, crafted(n, L, 44, lens=lens), L, lengths=True, variable_length=True)


def test_an_all_bare_input_has_no_entries(ctx):
    text = crafted(300, 50, 45, kinds=1)
    b = check_against_plain(ctx, text, 50)
    assert b.plus_info(0) == (300, 0, 0, 0)
    assert fmt.pack_plus(PR.entries(text)[0]) == b"scalce22" + bytes(8) + (300).to_bytes(8, "little")


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_a_line_of_65535_bytes_is_kept_and_one_more_is_an_error(ctx):
    heads = [b"@a", b"@b", b"@c"]
    rng = np.random.default_rng(51)
    long = ALPHABET[rng.integers(0, len(ALPHABET), size=65535)].tobytes()
    thirds = [b"+a", b"+" + long[:65534], b"+"]           # 65535 bytes and its newline: a stored entry of 65535
    b = check_against_plain(ctx, make_text(50, heads, thirds, 52), 50)
    assert b.plus_info(0)[1] == 65535
    thirds[1] = b"+" + long                               # 65536 bytes and its newline
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, make_text(50, heads, thirds, 52), 50, keep_plus=True)
    assert "[3]" in str(e.value) and "(ERROR) record 1: the '+' line is longer than 65535 bytes" in str(e.value)
    hip_compress(ctx, make_text(50, heads, thirds, 52), 50)   # without the option the text is the archive it was
    # a repeat of a long header line is one byte, however long the line
    heads[1] = b"@b " + long
    thirds[1] = b"+b " + long
    b = hip_compress(ctx, make_text(50, heads, thirds, 52), 50, keep_plus=True)
    check_plus(b, [[b"=", b"=", b""]])


@pytest.mark.parametrize("line", [b"", b"x", b" +", b"@r2"], ids=["empty", "letter", "space", "at"])
def test_a_third_line_that_does_not_begin_with_plus(line, ctx):
    heads = [b"@r%d" % r for r in range(5)]
    thirds = [b"+", b"+r1", line, b"+", b"+x"]
    text = make_text(50, heads, thirds, 53)
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, text, 50, keep_plus=True)
    assert "[3]" in str(e.value) and "(ERROR) record 2: the third line does not begin with '+'" in str(e.value)


def test_the_setter_and_the_calls_that_refuse_the_batch(ctx):
    from scalce_amd.pipeline import ShardPipeline
    for kw in (dict(fasta=True), dict(no_qualities=True)):
        with pytest.raises(host.ScalceError) as e:
            host.Batch(ctx, 50, max_reads=64, max_text=4096, keep_plus=True, **kw)
        assert "[1]" in str(e.value)
    text = crafted(40, 50, 61)
    t = device_bytes(text)
    b = host.Batch(ctx, 50, max_reads=64, max_text=len(text) + 64, bucket_set_size=1 << 20, keep_plus=True)
    comm = host.Comm(0, 1, 0, shm_name="/scalce_plus_%d" % os.getpid(), slot_bytes=1 << 20)
    try:
        with pytest.raises(host.ScalceError) as e:
            host.sharded_compress(comm, ctx, b, t.data_ptr(), len(text))
        assert "[1]" in str(e.value) and "--keep-plus" in str(e.value)
    finally:
        comm.close()
    with pytest.raises(RuntimeError) as e:
        ShardPipeline([b, host.Batch(ctx, 50, max_reads=64, max_text=4096)])
    assert "--keep-plus" in str(e.value)
    b.ingest(0, t.data_ptr(), len(text))
    with pytest.raises(host.ScalceError):
        b.text_offset(0, 3)


# ---- pieces -------------------------------------------------------------------------------------------------------------------
def run_pieces(ctx, text, L, cuts, nrec):
    """the text through scalce_batch_append in pieces that end at `cuts` (what a piece leaves over opens the next one)"""
    b = host.Batch(ctx, L, max_reads=nrec + 8, max_text=len(text) + 64, keep_plus=True)
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


def test_appended_pieces_cut_at_every_byte_of_a_small_text(ctx):
    heads = [b"@r0 a", b"@r1", b"@r2 x=1", b"@r3"]
    thirds = [b"+r0 a", b"+", b"+r2 x=2", b"+'"]
    text = make_text(6, heads, thirds, 21)
    ents = PR.entries(text)
    assert ents == [[b"=", b"", b"'r2 x=2", b"''"]]
    want = outputs(hip_compress(ctx, text, 6))
    for c in range(len(text) + 1):
        b = run_pieces(ctx, text, 6, [c], 4)
        check_plus(b, ents)
        assert outputs(b) == want, f"cut {c}"
    big = crafted(90, 50, 22)
    b = run_pieces(ctx, big, 50, [len(big) // 3, 2 * len(big) // 3 + 5], 90)
    check_plus(b, PR.entries(big))
    assert outputs(b) == outputs(hip_compress(ctx, big, 50))


# ---- mates --------------------------------------------------------------------------------------------------------------------
def test_mates_keep_their_own_lines_and_interleaved_text_gives_the_same(ctx):
    n, L1, L2 = 400, 100, 75
    rng = np.random.default_rng(31)
    h1 = [b"@p.%d/1 1:N:0:%d" % (r, r % 7) for r in range(n)]
    h2 = [b"@p.%d/2" % r + (b" 2:N:0" if r % 3 else b"") for r in range(n)]
    t1 = make_text(L1, h1, [third(r % 7, h1[r], r, rng) for r in range(n)], 32)
    t2 = make_text(L2, h2, [third((r * 3 + 1) % 7, h2[r], r, rng) for r in range(n)], 33)
    bp = check_against_plain(ctx, t1, L1, t2, L2)
    two = [bp.output(host.OUT_PLUS, m).tobytes() for m in range(2)]
    assert two[0] != two[1]
    r1, r2 = t1.split(b"\n"), t2.split(b"\n")
    il = b"".join(b"\n".join(r1[4 * k:4 * k + 4]) + b"\n" + b"\n".join(r2[4 * k:4 * k + 4]) + b"\n" for k in range(n))
    assert PR.entries(il, interleaved=True) == PR.entries(t1) + PR.entries(t2)
    t = device_bytes(il)
    bi = host.Batch(ctx, L1, max_reads=n + 8, max_text=len(il) + 64, paired=True, read_len2=L2, interleaved=True, keep_plus=True)
    bi.compress(t.data_ptr(), len(il))
    bi.finish()
    check_plus(bi, PR.entries(il, interleaved=True))
    assert [bi.output(host.OUT_PLUS, m).tobytes() for m in range(2)] == two
    assert outputs(bi, 2) == outputs(bp, 2)


def test_the_stream_outlives_the_lean_releases_beside_the_comments(ctx):
    n, L = 700, 100
    text = crafted(n, L, 71)
    perm = hip_compress(ctx, text, L).output(host.OUT_PERM, 0, np.uint32)
    t = device_bytes(text)
    b = host.Batch(ctx, L, max_reads=n + 8, max_text=len(text) + 64, keep_plus=True, keep_comments=True)
    b.set_lean(True)
    b.compress(t.data_ptr(), len(text))
    b.finish()
    assert b.output(host.OUT_PLUS, 0).tobytes() == PR.body(PR.entries(text)[0], perm)
    assert b.output(host.OUT_COMMENTS, 0).tobytes() == CR.body(CR.entries(text)[0], perm)


# ---- the insert pass alone ----------------------------------------------------------------------------------------------------
CANARY = 0xA5


def run_insert(ctx, text, off, body, out_bytes, pairs=None):
    """scalce_fastq_plus_window (or _pairs: pairs = the two read lengths) into a destination of exactly out_bytes with a canary
    behind it -> (text, offsets, verdict)"""
    import torch
    n = len(off) - 1
    d_text, d_ent = device_bytes(text), device_bytes(body if body else b"\0")
    d_off = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64)).to("cuda:0")
    d_out = torch.full((out_bytes + 4096,), CANARY, dtype=torch.uint8, device="cuda:0")
    d_out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    d_bad = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    if pairs is None:
        d_ws = torch.zeros(host.fastq_plus_ws_bytes(n, len(body)), dtype=torch.uint8, device="cuda:0")
        host.fastq_plus_window(ctx, n, d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(body), d_out.data_ptr(), out_bytes,
                               d_out_off.data_ptr(), d_bad.data_ptr(), d_ws.data_ptr())
    else:
        d_ws = torch.zeros(host.fastq_plus_pairs_ws_bytes(n, len(body)), dtype=torch.uint8, device="cuda:0")
        host.fastq_plus_window_pairs(ctx, pairs, n, d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(body), d_out.data_ptr(),
                                     out_bytes, d_out_off.data_ptr(), d_bad.data_ptr(), d_ws.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[out_bytes:] == CANARY).all(), "bytes written behind the destination"
    return got[:out_bytes].tobytes(), d_out_off.cpu().numpy().view(np.uint64), int(d_bad.cpu()[0])


def window(n, L, seed, lens=None):
    """a window's records as the passes in front of this one leave them (bare third lines), the entries to put back, and the
    text they came from"""
    whole = crafted(n, L, seed, lens=lens)
    lines = PR.bare(whole).split(b"\n")
    return [b"\n".join(lines[4 * r:4 * r + 4]) + b"\n" for r in range(n)], PR.entries(whole)[0], whole


def check_insert(ctx, recs, ents, whole):
    text = b"".join(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    want, want_off = PR.insert(text, off, ents)
    assert want == whole
    got, got_off, bad = run_insert(ctx, text, off, PR.body(ents), len(want))
    assert bad == 0
    assert (got_off == want_off).all()
    assert got == want


@pytest.mark.parametrize("n,L", [(1, 100), (2, 100), (281, 0), (281, 1), (281, 15), (281, 16), (281, 17), (281, 100), (41, 2498), (1400, 37)])
def test_insert_pass_against_the_restatement(n, L, ctx):
    """header lines of 1 to 40 bytes with every kind of line; the texts are no multiple of 16 KiB, so they end inside the last
    workgroup's span; 1400 records of 37 bases take several spans and begin on every phase of 16"""
    recs, ents, whole = window(n, L, 300 + n + L)
    assert len(whole) % 16384
    if n == 1400:
        assert {int(x) % 16 for x in np.cumsum([len(r) for r in recs])} == set(range(16)) and len(whole) > 5 * 16384
    check_insert(ctx, recs, ents, whole)


def test_insert_pass_of_one_record_of_each_class(ctx):
    for h, t in ((b"@r", b"+"), (b"@r", b"+r"), (b"@r", b"+q"), (b"@r 1:N:0 length=4", b"+r 1:N:0 length=4"), (b"@", b"+x")):
        whole = h + b"\nACGT\n" + t + b"\nIIII\n"
        check_insert(ctx, [PR.bare(whole)], PR.entries(whole)[0], whole)


def test_insert_pass_behind_the_strip(ctx):
    """records of different lengths, as the strip leaves them: the '+' is found from the header line and the record's size"""
    n, L = 600, 100
    rng = np.random.default_rng(81)
    lens = rng.permutation(np.concatenate([np.arange(L + 1), rng.integers(0, L + 1, size=n - L - 1)]))
    recs, ents, whole = window(n, L, 82, lens=lens)
    check_insert(ctx, recs, ents, whole)


def test_insert_pass_behind_the_comment_insert(ctx):
    """the comments are put in first by scalce_fastq_comment_window; a repeat then takes the header line with its comment"""
    import torch
    n, L = 500, 50
    recs, ents, whole = window(n, L, 83)
    kept = b"".join(recs)
    coms = CR.entries(kept)[0]
    stripped = CR.strip(kept)
    off = np.cumsum([0] + [len(r) - len(c) for r, c in zip(recs, coms)]).astype(np.uint64)
    cbody = CR.body(coms)
    d_text, d_ent = device_bytes(stripped), device_bytes(cbody)
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
    d_mid = torch.zeros(len(kept) + 64, dtype=torch.uint8, device="cuda:0")
    d_mid_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_ws = torch.zeros(host.fastq_comment_ws_bytes(n, len(cbody)), dtype=torch.uint8, device="cuda:0")
    host.fastq_comment_window(ctx, L, True, n, d_text.data_ptr(), d_off.data_ptr(), d_ent.data_ptr(), len(cbody), d_mid.data_ptr(),
                              d_mid_off.data_ptr(), d_bad.data_ptr(), d_ws.data_ptr())
    torch.cuda.synchronize()
    assert int(d_bad.cpu()[0]) == 0
    mid = d_mid.cpu().numpy().tobytes()[:len(kept)]
    assert mid == kept
    got, got_off, bad = run_insert(ctx, mid, d_mid_off.cpu().numpy().view(np.uint64), PR.body(ents), len(whole))
    assert bad == 0 and got == whole


def test_insert_pass_of_an_interleaved_window_with_two_read_lengths(ctx):
    n, L1, L2 = 300, 100, 37
    a, ea, wa = window(n, L1, 84)
    b, eb, wb = window(n, L2, 85)
    pairs = [x + y for x, y in zip(a, b)]
    ents = [e for xy in zip(ea, eb) for e in xy]
    text = b"".join(pairs)
    off = np.cumsum([0] + [len(p) for p in pairs]).astype(np.uint64)
    la, lb = wa.split(b"\n"), wb.split(b"\n")
    back = [b"\n".join(la[4 * k:4 * k + 4]) + b"\n" + b"\n".join(lb[4 * k:4 * k + 4]) + b"\n" for k in range(n)]
    want = b"".join(back)
    got, got_off, bad = run_insert(ctx, text, off, PR.body(ents), len(want), pairs=(L1, L2))
    assert bad == 0 and got == want
    assert (got_off == np.cumsum([0] + [len(p) for p in back]).astype(np.uint64)).all()


def test_malformed_entries_set_the_verdict_and_stay_inside_the_destination(ctx):
    recs, ents, whole = window(5, 50, 86)
    text = b"".join(recs)
    off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
    good = [b"=", b"", b"'abc", b"=", b"'="]
    assert run_insert(ctx, text, off, PR.body(good), len(PR.insert(text, off, good)[0]))[2] == 0
    for bad_ents in ([b"=", b"x", b"'abc", b"=", b""], [b"=x", b"", b"", b"", b""], [b"", b"", b"", b"", b"'"],
                     [b"+r", b"", b"", b"", b""]):
        # such records get a bare '+': the destination holds what the well-formed entries add and nothing more
        fixed = [e if e == b"=" or (e[:1] == b"'" and len(e) > 1) else b"" for e in bad_ents]
        want, want_off = PR.insert(text, off, fixed)
        got, got_off, bad = run_insert(ctx, text, off, PR.body(bad_ents), len(want))
        assert bad == 1, bad_ents
        assert got == want and (got_off == want_off).all()
    # too few, too many entries, no newline at the end
    for body in (b"=\n\n\n\n", b"=\n\n\n\n\n\n", b"=\n\n\n\n="):
        assert run_insert(ctx, text, off, body, len(text) + 400)[2] == 1, body
    # a destination that is too small takes nothing
    want = PR.insert(text, off, good)[0]
    got, _, bad = run_insert(ctx, text, off, PR.body(good), len(want) - 1)
    assert bad == 1 and got == bytes([CANARY]) * (len(want) - 1)
