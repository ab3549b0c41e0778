"""-m gpu: reads of different lengths through the C ABI (params variable_length).

Identity: a variable-length text and its N-padded twin give equal SCALCE_OUT_READS, _NAMES, _QUAL, _TABLE and _PERM, and
SCALCE_OUT_LENGTHS is (L - length)[perm] -- the pad pass in front of the ingest is the only thing that differs.  Errors are
SCALCE_ERR_* with a message.  The strip pass of the decode side is called on its own against a numpy restatement."""
import numpy as np
import pytest

import decode_ref as R
import varlen_util as V
from gpu_util import device_bytes, hip_compress
from scalce_amd import host

pytestmark = pytest.mark.gpu
STREAMS = (("reads", host.OUT_READS), ("names", host.OUT_NAMES), ("qual", host.OUT_QUAL), ("table", host.OUT_TABLE))


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def outputs(b, mates=1):
    out = {}
    for m in range(mates):
        for name, which in STREAMS:
            out[name, m] = b.output(which, 0 if which == host.OUT_NAMES else m).tobytes()
    out["perm"] = b.output(host.OUT_PERM, 0, np.uint32).copy()
    return out


def check_identity(ctx, L, lens, seed, names=None, **kw):
    var, pad, _ = V.texts(L, lens, seed, names=names)
    bv = hip_compress(ctx, var, L, variable_length=True, **kw)
    bp = hip_compress(ctx, pad, L, **kw)
    ov, op = outputs(bv), outputs(bp)
    assert bv.n_reads == bp.n_reads == len(lens)
    for key in op:
        if key == "perm":
            assert (ov[key] == op[key]).all(), "permutation"
        else:
            assert ov[key] == op[key], key
    got = bv.output(host.OUT_LENGTHS, 0, np.uint16)
    assert (got == (L - np.asarray(lens))[op["perm"]]).all(), "lengths in output order"
    assert bp.output_ptr(host.OUT_LENGTHS, 0)[1] == 0  # a fixed-length run has none
    return var, pad


# ---- identity -------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_byte_phase(ctx):
    """L = 100, lengths 0 .. 100 all present, shuffled: record starts of the text fall on every phase of 16"""
    lens = V.lengths_covering(700, 100, 1)
    var, _ = check_identity(ctx, 100, lens, 11)
    starts = np.cumsum([0] + [len(r) for r in V.records_of(var)])[:-1]
    assert set(starts % 16) == set(range(16)) and set(lens) == set(range(101))


@pytest.mark.parametrize("L", [37, 16, 161, 300])
def test_read_lengths_that_pick_other_paths(L, ctx):
    """37: no multiple of 4 or 16; 16 and 161: the two ingest routes of the padded text (one pass, indexed); 300: two-byte
    entries and two bytes of end metadata"""
    check_identity(ctx, L, V.lengths_covering(400, L, L), 20 + L)


def test_all_reads_at_full_length(ctx):
    check_identity(ctx, 100, np.full(300, 100), 31)


def test_all_reads_empty_but_one(ctx):
    lens = np.zeros(300, dtype=np.int64)
    lens[137] = 100
    check_identity(ctx, 100, lens, 32)


def test_names_of_1_15_16_and_255_characters(ctx):
    n = 320
    lens = V.lengths_covering(n, 100, 3)
    digits = lambda i, w: (b"%0*d" % (w, i))  # noqa: E731
    names = []
    for i in range(n):
        w = (1, 15, 16, 255)[i % 4]
        # one character: 80 distinct ones; else the index, zero padded to the width
        names.append(bytes([48 + i // 4]) if w == 1 else digits(i, w))
    check_identity(ctx, 100, lens, 33, names=names)


@pytest.fixture(scope="module")
def tile_text():
    """a text that spans three 16 KiB index tiles with a record across each tile edge"""
    L = 100
    lens = V.lengths_covering(330, L, 4)
    var, pad, names = V.texts(L, lens, 34)
    ends = np.cumsum([len(r) for r in V.records_of(var)])
    assert len(var) > 2 * 16384 and 16384 not in ends and 32768 not in ends
    return L, lens, var, pad, names


def test_text_over_three_index_tiles(ctx, tile_text):
    L, lens, _, _, _ = tile_text
    check_identity(ctx, L, lens, 34)


def test_appended_pieces_cut_inside_one_record(ctx, tile_text):
    """the same text through scalce_batch_append in two pieces, the first cut inside one chosen record: thinned to every third
    offset of the record plus both ends of each of its four lines (the first and last byte of the line and its newline)"""
    L, lens, var, pad, names = tile_text
    want = outputs(hip_compress(ctx, pad, L))
    recs = V.records_of(var)
    k = next(i for i in range(len(recs) // 2, len(recs)) if 30 < lens[i] < 90)
    start = sum(len(r) for r in recs[:k])
    rec = recs[k]
    cuts = set(range(0, len(rec) + 1, 3))
    at = 0
    for line in rec[:-1].split(b"\n"):
        cuts |= {at, at + 1, at + len(line) - 1, at + len(line), at + len(line) + 1} & set(range(len(rec) + 1))
        at += len(line) + 1
    b = host.Batch(ctx, L, max_reads=len(recs) + 8, max_text=len(var) + 64, variable_length=True)
    for c in sorted(cuts):
        cut = start + c
        b.reset()
        first = device_bytes(var[:cut]) if cut else None
        used, _ = b.append(first.data_ptr() if cut else None, cut)
        whole = sum(len(r) for r in recs[:k + (1 if c == len(rec) else 0)])
        assert used == whole, f"cut {c}: consumed counts the caller's bytes, whole records only"
        rest = device_bytes(var[used:])
        used2, _ = b.append(rest.data_ptr(), len(var) - used, final=True)
        assert used2 == len(var) - used
        b.order(); b.emit(); b.entropy(); b.finish()
        got = outputs(b)
        for key in want:
            assert (got[key] == want[key]).all() if key == "perm" else got[key] == want[key], f"cut {c}: {key}"
        assert (b.output(host.OUT_LENGTHS, 0, np.uint16) == (L - lens)[want["perm"]]).all(), f"cut {c}"


def test_paired_with_independent_lengths(ctx):
    n, L1, L2 = 500, 100, 75
    len1, len2 = V.lengths_covering(n, L1, 5), V.lengths_covering(n, L2, 6)
    v1, p1, _ = V.texts(L1, len1, 35, prefix="p.", suffix="/1")
    v2, p2, _ = V.texts(L2, len2, 36, prefix="p.", suffix="/2")
    bv = hip_compress(ctx, v1, L1, v2, L2, variable_length=True)
    bp = hip_compress(ctx, p1, L1, p2, L2)
    ov, op = outputs(bv, 2), outputs(bp, 2)
    for key in op:
        assert (ov[key] == op[key]).all() if key == "perm" else ov[key] == op[key], key
    assert (bv.output(host.OUT_LENGTHS, 0, np.uint16) == (L1 - len1)[op["perm"]]).all()
    assert (bv.output(host.OUT_LENGTHS, 1, np.uint16) == (L2 - len2)[op["perm"]]).all(), "mate 2 follows mate 1's order"


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_record_longer_than_L_is_an_error(ctx):
    lens = V.lengths_covering(300, 50, 7)
    lens[211] = 57
    var, _, _ = V.texts(60, lens, 37)
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, var, 50, variable_length=True)
    assert "[3]" in str(e.value) and "record 211 holds 57 bases" in str(e.value) and "--max-length" in str(e.value)


def test_sequence_and_quality_lines_that_differ_are_an_error(ctx):
    var, _, _ = V.texts(50, V.lengths_covering(300, 50, 8, lo=2), 38)
    recs = V.records_of(var)
    name, seq, plus, qual = recs[123][:-1].split(b"\n")
    recs[123] = name + b"\n" + seq + b"\n" + plus + b"\n" + qual[:-1] + b"\n"
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, b"".join(recs), 50, variable_length=True)
    assert "[3]" in str(e.value) and "record 123" in str(e.value) and "differ" in str(e.value)


@pytest.mark.parametrize("kw", [dict(fasta=True), dict(no_qualities=True), dict(paired=True, interleaved=True)], ids=["fasta", "no_qualities", "interleaved"])
def test_flag_is_refused_with_other_record_shapes(kw, ctx):
    with pytest.raises(host.ScalceError) as e:
        host.Batch(ctx, 50, max_reads=64, max_text=4096, variable_length=True, **kw)
    assert "[1]" in str(e.value) and "variable-length" in str(e.value)


def test_without_the_flag_a_short_read_is_the_error_it_was(ctx):
    var, _, _ = V.texts(50, V.lengths_covering(300, 50, 9), 39)
    with pytest.raises(host.ScalceError) as e:
        hip_compress(ctx, var, 50)
    assert "read_length" in str(e.value)


# ---- the strip pass alone ------------------------------------------------------------------------------------------------
def edge_lengths(n, L, rng):
    """the length sets of a window of n records: 0, 1, L - 1 and L at both of its ends (small windows: one set per edge value)"""
    edge = [0, 1, L - 1, L]
    if n == 1:
        return [np.array([e]) for e in edge]
    if n == 2:
        return [np.array(p) for p in ((0, 1), (L - 1, L), (1, L - 1), (L, 0))]
    lens = rng.integers(0, L + 1, size=n)
    lens[:4] = edge
    lens[-4:] = edge[::-1]
    return [lens]


@pytest.mark.parametrize("named", [True, False], ids=["names", "library"])
@pytest.mark.parametrize("L", [100, 300])
@pytest.mark.parametrize("n", [1, 2, 257])
def test_strip_window_alone(n, L, named, ctx):
    """scalce_fastq_records_window on a crafted window of bare records, then the strip call: lengths 0, 1, L - 1 and L at both
    ends of the window, stored names and made-up ones (-n); text and new record offsets against numpy"""
    import torch
    import test_gpu_decode_entries as E
    rng = np.random.default_rng(n * 1000 + L)
    for lens in edge_lengths(n, L, rng):
        reads = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)]) for _ in range(n)]
        q = rng.integers(1, 63, size=(n, L)).astype(np.uint8)
        for i in range(n):
            q[i, lens[i]:] = 0   # the pad: an N, quality symbol 0
        names = [b"r%d" % i + b"x" * int(rng.integers(0, 30)) for i in range(n)] if named else None
        padded, offs = R.text_of(reads, q, names if named else (b"lib", 7), 33, 0)
        d_q = E.In(q.tobytes(), 0)
        out = E.Out(len(padded), 0)
        got_offs = E.run_window(ctx, L, R.pack_records(reads, None, None, L, 0), 0, n, out.ptr, first=0 if named else 7, d_qual=d_q.ptr,
                                names=names, library=None if named else b"lib", want_offsets=True)
        assert out.region().tobytes() == padded and got_offs == offs
        width = 1 if L <= 255 else 2
        entries = (L - lens).astype("<u1" if width == 1 else "<u2").tobytes()
        recs = V.records_of(padded)
        want = b"".join(V.cut_to_lengths(r, {r[1:r.index(b"\n")]: int(k)}) for r, k in zip(recs, lens))
        want_offs = [0] + [int(v) for v in np.cumsum([len(r) - 2 * (L - int(k)) for r, k in zip(recs, lens)])]
        assert len(want) == want_offs[-1]
        d_roff, d_ent = E.dev_u64(offs), E.In(entries, 0)
        stripped = E.Out(len(want), 0)
        new_off = torch.full((n + 3,), -1, dtype=torch.int64, device=E.DEV)
        ws = torch.zeros(host.fastq_strip_ws_bytes(n), dtype=torch.uint8, device=E.DEV)
        host.fastq_strip_window(ctx, L, n, out.ptr, d_roff.data_ptr(), d_ent.ptr, width, stripped.ptr, new_off.data_ptr() + 8, ws.data_ptr())
        torch.cuda.synchronize()
        assert stripped.region().tobytes() == want, list(lens[:4])
        h = new_off.cpu().numpy()
        assert h[0] == -1 and h[-1] == -1 and [int(v) for v in h[1:-1]] == want_offs
