"""-m gpu: the tokenizer's walks on every core-table shape that selects them (tests/bigtable.py SHAPES).

The loaded table alone decides the walk (scalce_patterns_walk): the k-mer walk, with T7 when a core is shorter than 8
bases, or the anchor walk of K bases.  Each test asserts the walk its table is built to select, then compares the
device's tokens (bucket, last base) and order with the oracle's trie walk read by read, on reads whose cores sit where
the kernels have corners: base 0, the last base (the last rows of the batch too), every offset within a 32-bit word of
the packed row, across the 128-position segments of the anchor probes, one base short of an anchor, ties."""
import os
import subprocess

import numpy as np
import pytest

import bigtable as B
import oraclelib as O
from gpu_util import device_bytes
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scalce_amd", "bin", "scalce")
ANCHOR_SHAPES = [s for s in B.SHAPES if B.shape(s).walk[0] == "anchor"]
N_READS = 6000
_CTX, _TRIE = {}, {}


def table(name):
    """(Table, device context, oracle trie), built once per module"""
    t = B.shape(name)
    if name not in _CTX:
        _CTX[name] = host.Context(0, patterns_text=t.blob) if t.text else host.Context(0, patterns_bin=t.blob)
        _TRIE[name] = O.Trie(text=t.blob) if t.text else O.Trie(blob=t.blob)
    return t, _CTX[name], _TRIE[name]


def anchor_len(t):
    return t.walk[1] or 8


def run(ctx, bases):
    n, L = bases.shape
    fq = synth.fastq_bytes_fast(bases, np.full(bases.shape, ord("I"), dtype=np.uint8))
    d = device_bytes(fq)
    b = host.Batch(ctx, L, n + 8, len(fq) + 64)
    b.compress(d.data_ptr(), len(fq))
    b.finish()
    b._keep = d
    return b


def check_against_oracle(b, trie, bases, what):
    pat, end = trie.tokenize(bases)
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    bad = np.flatnonzero((tok[:, 0] != pat) | (tok[:, 1] != end))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(bases)} reads differ, first {bad[:4]}: device "
                           f"{tok[bad[:4]].tolist()} oracle {list(zip(pat[bad[:4]], end[bad[:4]]))} ({b.stats()})")
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    assert (perm == trie.order(bases, pat, end)).all(), f"{what}: order differs"
    return pat, end


@pytest.mark.parametrize("name", B.SHAPES)
def test_walk_of_every_shape(name):
    t, ctx, trie = table(name)
    assert ctx.walk == t.walk, f"{name}: table selects {ctx.walk}, built for {t.walk}"
    assert ctx.n_patterns == len(t.cores) == trie.n_patterns
    if t.note.startswith("states=="):
        assert ctx.n_states == int(t.note.split("==")[1])
    elif t.note == "states>=1M":
        assert ctx.n_states >= 1_000_000


@pytest.mark.parametrize("name", B.SHAPES)
def test_tokens_and_order_at_every_read_length(name):
    """all read lengths of the shape in one test (one table, eleven batches): tokens and order equal the oracle's"""
    t, ctx, trie = table(name)
    assert ctx.walk == t.walk
    found = 0
    for L in B.read_lengths(anchor_len(t)):
        bases = B.corner_reads(t.cores, L, N_READS, seed=L)
        b = run(ctx, bases)
        pat, _ = check_against_oracle(b, trie, bases, f"{name} L={L}")
        found += int((pat >= 0).sum())
    assert found > N_READS   # (the planted cores are found: the comparison is not one of empty tokens)


def test_longest_core_on_the_last_base_of_the_last_reads():
    """a batch whose every read ends in a core of 15..17 bases behind the anchor (single records that compare up to
    two words past base i + 1): the last rows of the buffer included"""
    t, ctx, trie = table("single")
    assert ctx.walk == ("anchor", 12)
    for L in (28, 29, 31, 32, 33, 100, 129):
        cores = [c for c in t.cores if len(c) in (27, 28, 29) and len(c) <= L]
        rng = np.random.default_rng(L)
        bases = B.ACGT[rng.integers(0, 4, size=(1000, L))]
        for r in range(len(bases)):
            c = cores[int(rng.integers(0, len(cores)))]
            bases[r, L - len(c):] = np.frombuffer(c.encode(), dtype=np.uint8)
        b = run(ctx, bases)
        pat, end = check_against_oracle(b, trie, bases, f"last base L={L}")
        assert (end == L).all()


TIE_SHAPES = ANCHOR_SHAPES + ["short_t7"]


@pytest.mark.parametrize("name", TIE_SHAPES)
@pytest.mark.parametrize("mode", ["0", "700", "700:two_launches", "sweeps8"])
def test_tie_reads(name, mode, monkeypatch):
    """reads that each hold two of a few cores of one length: ties decided by the counts of the reads in front, through
    the global sweeps, windows of 700 tie reads (one or two launches), and the bounded sweeps with the sequential way out"""
    if mode == "sweeps8":
        monkeypatch.setenv("SCALCE_TIE_MAX_SWEEPS", "8")
    else:
        monkeypatch.setenv("SCALCE_TIE_WINDOW", mode)
    t, ctx, trie = table(name)
    assert ctx.walk == t.walk
    bases = B.tie_reads(t.cores, 100, 20_000, seed=len(name))
    b = run(ctx, bases)
    check_against_oracle(b, trie, bases, f"{name} ties {mode}")
    assert b.stats()["tie_reads"] > 10_000
    if mode != "sweeps8":   # the hook selected the path the case is named after
        plan = b.tie_plan()
        assert plan["path"] == {"0": 3, "700": 1, "700:two_launches": 2}[mode] and plan["window"] == (0 if mode == "0" else 700)


@pytest.mark.parametrize("name", TIE_SHAPES)
def test_pieces_equal_one_shard(name):
    """the same input appended in pieces (the counts of earlier pieces carry into the ties of later ones) gives the
    tokens and order of one shard, which are the oracle's"""
    from test_gpu_stream import feed_in_pieces
    t, ctx, trie = table(name)
    assert ctx.walk == t.walk
    n, L = 12_000, 129
    bases = np.concatenate([B.corner_reads(t.cores, L, n // 2, seed=9), B.tie_reads(t.cores, L, n // 2, seed=10)])
    bases = bases[np.random.default_rng(11).permutation(n)]
    whole = run(ctx, bases)
    check_against_oracle(whole, trie, bases, f"{name} one shard")
    fq = synth.fastq_bytes_fast(bases, np.full(bases.shape, ord("I"), dtype=np.uint8))
    piece = len(fq) // 6 + 17
    b = host.Batch(ctx, L, n // 3, piece + 64)
    assert feed_in_pieces(b, [fq], piece) >= 6 and b.n_reads == n
    b.order(); b.emit(); b.entropy(); b.finish()
    for which in (host.OUT_TOKENS, host.OUT_PERM):
        assert (whole.output(which, 0) == b.output(which, 0)).all(), (name, which)


def test_cli_pairs_with_anchor_text_table(tmp_path):
    """-r through the command line with an anchor table given as a text list (-P): the oracle CLI's files"""
    t, ctx, _ = table("long_text_anchor")
    assert ctx.walk == ("anchor", 12)
    (tmp_path / "p.txt").write_bytes(t.blob)
    n, L = 6000, 150
    rng = np.random.default_rng(5)
    for m in (1, 2):
        bases = B.corner_reads(t.cores, L, n, seed=40 + m)
        quals = rng.integers(35, 74, size=bases.shape).astype(np.uint8)
        (tmp_path / f"in_{m}.fq").write_bytes(synth.fastq_bytes_fast(bases, quals, prefix="p.", suffix=f"/{m}"))
    r = subprocess.run([CLI, "-r", "-c", "no", "-o", str(tmp_path / "hip"), str(tmp_path / "in_1.fq"), "-P",
                        str(tmp_path / "p.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    O.orc_cli("compress", "-P", tmp_path / "p.txt", tmp_path / "in_1.fq", tmp_path / "orc", "-r")
    for m in (1, 2):
        for ext in "nrq":
            a = (tmp_path / f"orc_{m}.scalce{ext}").read_bytes()
            h = (tmp_path / f"hip_{m}.scalce{ext}").read_bytes()
            assert a == h, f".scalce{ext} mate {m}: {len(h)} vs {len(a)} bytes"


def test_core_of_128_bases_is_refused():
    """the device takes cores of up to 127 bases; a longer one is a loud error, not a table that quietly differs"""
    ok = host.Context(0, patterns_text=b"ACGTACGTAC\n" + b"G" * 127 + b"\n")
    assert ok.n_patterns == 2
    with pytest.raises(host.ScalceError, match="127"):
        host.Context(0, patterns_text=b"ACGTACGTAC\n" + b"G" * 128 + b"\n")
