"""Compression without qualities: FASTA input (-f) and FASTQ whose qualities are dropped (-Q), end to end on the device.

The reference writes the same .scalcer / .scalcen bytes with and without qualities whenever the spill-chunk cuts coincide
(neither the order nor the record bytes depend on qualities), and a .scalceq that holds "scalce22" + the int64 phred offset
and nothing else (compress.cpp:249,296; arithmetic.cpp:319-339).  The expected bytes therefore come from the hashes the
reference wrote for the same inputs with qualities (tests/golden/files.json) and from that header rule.
"""
import gzip
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import filecases as F
from scalce_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "files.json")))
MAGIC = b"scalce22"


def sha(b):
    return hashlib.sha256(b).hexdigest()


def run(*args, ok=True, env=None):
    r = subprocess.run([F.SCALCE, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def to_fasta(text):
    """FASTQ text -> FASTA: '>' + name, then the sequence; the '+' and quality lines are dropped"""
    lines = text.split(b"\n")
    assert len(lines) % 4 == 1 and lines[-1] == b""
    out = []
    for i in range(0, len(lines) - 1, 4):
        out += [b">" + lines[i][1:], lines[i + 1]]
    return b"\n".join(out) + b"\n"


def case_inputs(name, d, fasta=False):
    """the case's input files in d (FASTA versions under -f); returns the input paths of mate 1"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    F.write_inputs(name, d)
    paths = [os.path.join(d, f) for f in F.input_names(name)]
    if fasta:
        for p in paths:
            mate2 = os.path.join(d, os.path.basename(p).replace("_1", "_2"))
            for q in ([p, mate2] if F.paired(name) else [p]):
                raw = open(q, "rb").read()
                text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
                data = to_fasta(text)
                open(q, "wb").write(gzip.compress(data, 1) if raw[:2] == b"\x1f\x8b" else data)
    return paths


def case_flags(name):
    """the case's flags in CLI spelling (-B in M); -p and -s stay: they change nothing but the sample without qualities"""
    flags = list(F.CASES[name]["flags"])
    if "-B" in flags:
        i = flags.index("-B")
        flags[i + 1] = "%dM" % (int(flags[i + 1]) >> 20)
    if "-c" not in flags:
        flags += ["-c", "no"]
    return flags


def table_flags(name, d):
    return ["-P", os.path.join(str(d), "p.txt")] if F.CASES[name].get("ptxt") else ["--patterns-bin", F.PBIN]


def compress(name, d, prefix, mode, extra=(), inputs=None, env=None, ok=True):
    ins = inputs if inputs is not None else [os.path.join(str(d), f) for f in F.input_names(name)]
    return run(mode, *case_flags(name), *extra, "-o", os.path.join(str(d), prefix), *ins, *table_flags(name, d), ok=ok, env=env)


def mates(name):
    return (1, 2) if F.paired(name) else (1,)


def phred_of(name):
    if F.CASES[name].get("phred64"):
        return 64
    return 33


# ---- 1, 2: the archive is the reference's ------------------------------------------------------------------------------
CASES_Q = ["se100", "se100_nlib", "se100_ptxt", "se100_gz", "se100_letters", "se100_phred64", "pe150", "pe150_gz_nlib", "multi"]


@pytest.mark.parametrize("mode", ["-Q", "-f"])
@pytest.mark.parametrize("name", CASES_Q)
def test_archive_matches_reference(name, mode, tmp_path):
    case_inputs(name, tmp_path, fasta=mode == "-f")
    compress(name, tmp_path, "nq", mode)
    offset = 64 if mode == "-f" else phred_of(name)  # -f samples nothing: the statistics stay zero (qualities.cpp:91-101)
    for m in mates(name):
        for ext in "rn":
            got = F.content(tmp_path / f"nq_{m}.scalce{ext}")
            assert sha(got) == GOLD[name][f"{m}.scalce{ext}"], f"{name} {mode} mate {m} .scalce{ext}"
        q = open(tmp_path / f"nq_{m}.scalceq", "rb").read()
        assert q == MAGIC + struct.pack("<q", offset), f"{name} {mode} mate {m} .scalceq: {q[:32]!r}"


@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_header_only_quality_file_with_A_is_gzip(mode, tmp_path):
    name = "se100"
    case_inputs(name, tmp_path, fasta=mode == "-f")
    run(mode, "-A", "-c", "gz", "-o", tmp_path / "a", *[tmp_path / f for f in F.input_names(name)], "--patterns-bin", F.PBIN)
    raw = open(tmp_path / "a_1.scalceq", "rb").read()
    assert raw[:2] == b"\x1f\x8b"
    assert gzip.decompress(raw) == MAGIC + struct.pack("<q", 64 if mode == "-f" else 33)
    assert sha(F.content(tmp_path / "a_1.scalcer")) == GOLD["se100_A"]["1.scalcer"]


# ---- 3: -B cuts on records without quality bytes -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_spill_chunks_without_quality_bytes(mode, tmp_path):
    """names 100 characters longer weigh exactly what the qualities weighed: the cuts are the reference's of se100_B"""
    name = "se100_B"
    F.write_inputs(name, tmp_path)
    text = open(tmp_path / "in_1.fq", "rb").read()
    lines = text.split(b"\n")
    for i in range(0, len(lines) - 1, 4):
        lines[i] += b"x" * 100
    text = b"\n".join(lines)
    open(tmp_path / "in_1.fq", "wb").write(to_fasta(text) if mode == "-f" else text)
    run(mode, "-B", "1M", "-c", "no", "-o", tmp_path / "b", tmp_path / "in_1.fq", "--patterns-bin", F.PBIN)
    assert sha(open(tmp_path / "b_1.scalcer", "rb").read()) == GOLD[name]["1.scalcer"]


# ---- 4: streaming = resident ----------------------------------------------------------------------------------------------
STREAM_CASES = ["se", "pe", "two_files_gz", "chunks"]


@pytest.mark.parametrize("piece", [40000, 700000])
@pytest.mark.parametrize("case", STREAM_CASES)
@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_streaming_equals_one_piece(mode, case, piece, tmp_path):
    n, L = 30000, 100
    b1, q1 = synth.reads_and_quals(n, L, seed=71, n_frac=0.003, dup_frac=0.1)
    conv = to_fasta if mode == "-f" else (lambda t: t)
    files = [tmp_path / "in_1.fq"]
    fq = synth.fastq_bytes_fast(b1, q1, prefix="p." if case == "pe" else "s.", suffix="/1" if case == "pe" else "")
    if case == "two_files_gz":
        cut = fq.index(b"\n@s.17001\n") + 1
        open(files[0], "wb").write(gzip.compress(conv(fq[:cut]), 1))
        files.append(tmp_path / "more_1.fq")
        open(files[1], "wb").write(conv(fq[cut:]))
    else:
        open(files[0], "wb").write(conv(fq))
    flags = ["-c", "no"]
    if case == "pe":
        b2, q2 = synth.reads_and_quals(n, L, seed=72)
        recs = [b"@p.%d/2 " % i + b"c" * 60 + b"\n" + b2[i].tobytes() + b"\n+\n" + q2[i].tobytes() + b"\n" for i in range(n)]
        open(tmp_path / "in_2.fq", "wb").write(conv(b"".join(recs)))
        flags.append("-r")
    if case == "chunks":
        flags += ["-B", "1M"]
    env = dict(os.environ, SCALCE_PIECE_BYTES=str(piece))
    r = run(mode, *flags, "-o", tmp_path / "st", *files, "--patterns-bin", F.PBIN, env=env)
    assert "pieces streamed" in r.stderr
    run(mode, *flags, "-o", tmp_path / "one", *files, "--patterns-bin", F.PBIN)
    for m in ((1, 2) if case == "pe" else (1,)):
        for ext in "nrq":
            a = open(tmp_path / f"one_{m}.scalce{ext}", "rb").read()
            b = open(tmp_path / f"st_{m}.scalce{ext}", "rb").read()
            assert a == b, f"{mode} {case} piece {piece} .scalce{ext} mate {m}"


# ---- 6: round trip --------------------------------------------------------------------------------------------------------
def normalised(seq):
    """what a base stored without its quality decodes to: upper case, every letter but ACGT -> A (getval, const.cpp:47-49)"""
    s = np.frombuffer(seq.upper(), dtype=np.uint8).copy()
    s[~np.isin(s, np.frombuffer(b"ACGT", dtype=np.uint8))] = ord("A")
    return s.tobytes()


def fastq_records(text):
    lines = text.split(b"\n")
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]


def expected_two_line(order_fastq, input_text, library=None):
    """archive order from a restored FASTQ (names unique); bases from the input read of the same name"""
    seqs = {nm.split(b" ")[0]: sq for nm, sq in fastq_records(input_text)}
    out = []
    for k, (nm, _) in enumerate(fastq_records(order_fastq)):
        shown = nm if library is None else b"%s.%d" % (library.encode(), k)
        out.append(b"@" + shown + b"\n" + normalised(seqs[nm]) + b"\n")
    return b"".join(out)


def reference_order(name, d):
    """the run with qualities, restored: its FASTQ is pinned by files.json, its name lines give the archive order"""
    F.run_tool("hip", name, d, "withq")
    F.run_decompress("hip", name, d, "withq", "withq_back")
    out = []
    for m in mates(name):
        t = open(os.path.join(str(d), f"withq_back_{m}.fastq"), "rb").read()
        assert sha(t) == GOLD[name][f"{m}.fastq"]
        out.append(t)
    return out


@pytest.mark.parametrize("mode", ["-Q", "-f"])
@pytest.mark.parametrize("name", ["se100", "se100_letters", "pe150", "multi"])
def test_round_trip(name, mode, tmp_path):
    texts = F.write_inputs(name, tmp_path)
    order = reference_order(name, tmp_path)
    src = tmp_path / "src"
    case_inputs(name, src, fasta=mode == "-f")
    compress(name, src, "nq", mode)
    run("-d", mode, *(["-r"] if F.paired(name) else []), "-o", tmp_path / "back", src / "nq_1.scalcen", "--patterns-bin", F.PBIN)
    for i, m in enumerate(mates(name)):
        got = open(tmp_path / f"back_{m}.fastq", "rb").read()
        want = expected_two_line(order[i], texts[i])
        assert got == want, f"{name} {mode} mate {m}: {len(got)} vs {len(want)} bytes"


@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_round_trip_library_names_and_split(mode, tmp_path):
    name = "se100"
    texts = F.write_inputs(name, tmp_path)
    order = reference_order(name, tmp_path)
    src = tmp_path / "src"
    case_inputs(name, src, fasta=mode == "-f")
    run(mode, "-n", "lib", "-c", "no", "-o", src / "nq", src / "in_1.fq", "--patterns-bin", F.PBIN)
    run("-d", mode, "-S", "7000", "-o", tmp_path / "back", src / "nq_1.scalcen", "--patterns-bin", F.PBIN)
    want = expected_two_line(order[0], texts[0], library="lib")
    parts = []
    for part in range(1, 6):
        t = open(tmp_path / f"back.{part}_1.fastq", "rb").read()
        assert t.count(b"\n") == 2 * min(7000, 30000 - 7000 * (part - 1))
        parts.append(t)
    assert not os.path.exists(tmp_path / "back.6_1.fastq")
    assert b"".join(parts) == want


# ---- 5: read lengths of every ingest route ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["-Q", "-f"])
@pytest.mark.parametrize("L", [20, 200, 300])
def test_length_routes(L, mode, tmp_path):
    """L = 20: the tile kernel; 200: the indexed fallback (161 .. 300); 300: two-byte end markers (L > 255)"""
    n = 6000
    bases, quals = synth.reads_and_quals(n, L, seed=80 + L, n_frac=0.01, dup_frac=0.2)
    fq = synth.fastq_bytes_fast(bases, quals)
    open(tmp_path / "q_1.fq", "wb").write(fq)
    open(tmp_path / "x_1.fq", "wb").write(to_fasta(fq) if mode == "-f" else fq)
    run("-c", "no", "-o", tmp_path / "withq", tmp_path / "q_1.fq", "--patterns-bin", F.PBIN)
    run(mode, "-c", "no", "-o", tmp_path / "nq", tmp_path / "x_1.fq", "--patterns-bin", F.PBIN)
    assert open(tmp_path / "nq_1.scalcer", "rb").read() == open(tmp_path / "withq_1.scalcer", "rb").read()
    assert open(tmp_path / "nq_1.scalcen", "rb").read() == open(tmp_path / "withq_1.scalcen", "rb").read()
    run("-d", "-o", tmp_path / "withq_back", tmp_path / "withq_1.scalcen", "--patterns-bin", F.PBIN)
    run("-d", mode, "-o", tmp_path / "back", tmp_path / "nq_1.scalcen", "--patterns-bin", F.PBIN)
    want = expected_two_line(open(tmp_path / "withq_back_1.fastq", "rb").read(), fq)
    assert open(tmp_path / "back_1.fastq", "rb").read() == want


# ---- 7: nothing quality-side runs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_qualities", "fasta"])
def test_batch_launches_nothing_quality_side(kind, patterns_blob):
    import torch
    from scalce_amd import host
    ctx = host.Context(0, patterns_bin=patterns_blob)
    bases, quals = synth.reads_and_quals(20000, 100, seed=5, dup_frac=0.1, n_frac=0.002)
    fq = synth.fastq_bytes_fast(bases, quals)
    text = to_fasta(fq) if kind == "fasta" else fq
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    ref = host.Batch(ctx, 100, 20008, len(fq) + 64)
    ref.compress(torch.frombuffer(bytearray(fq), dtype=torch.uint8).to("cuda:0").data_ptr(), len(fq))
    ref.finish()
    b = host.Batch(ctx, 100, 20008, len(text) + 64, **{kind: True})
    b.stage_reset(True)
    b.compress(t.data_ptr(), len(text))
    b.finish()
    st = b.stage_ms()
    stages = list(st)
    assert st[stages[1]][1] == 0 and st[stages[5]][1] == 0, st
    assert st[stages[0]][1] > 0 and st[stages[4]][1] > 0, st
    assert b.qual_bytes(0) == 0
    assert (b.output(host.OUT_PERM, 0, np.uint32) == ref.output(host.OUT_PERM, 0, np.uint32)).all()
    assert (b.output(host.OUT_READS, 0) == ref.output(host.OUT_READS, 0)).all()
    assert (b.output(host.OUT_NAMES, 0) == ref.output(host.OUT_NAMES, 0)).all()


# ---- 8: errors --------------------------------------------------------------------------------------------------------
def test_errors(tmp_path):
    bases, quals = synth.reads_and_quals(500, 60, seed=9)
    fq = synth.fastq_bytes_fast(bases, quals)
    fa = to_fasta(fq)
    # wrapped FASTA: the sequence over two lines
    recs = fa.split(b"\n")
    wrapped = b"".join(recs[i] + b"\n" + recs[i + 1][:30] + b"\n" + recs[i + 1][30:] + b"\n" for i in range(0, len(recs) - 1, 2))
    open(tmp_path / "w_1.fa", "wb").write(wrapped)
    r = run("-f", "-c", "no", "-o", tmp_path / "w", tmp_path / "w_1.fa", "--patterns-bin", F.PBIN, ok=False)
    assert r.returncode != 0 and "(ERROR)" in r.stderr, r.stderr[-500:]
    # a FASTA mate that ends early
    open(tmp_path / "p_1.fa", "wb").write(fa)
    open(tmp_path / "p_2.fa", "wb").write(b"\n".join(fa.split(b"\n")[:-21]) + b"\n")
    r = run("-f", "-r", "-c", "no", "-o", tmp_path / "p", tmp_path / "p_1.fa", "--patterns-bin", F.PBIN, ok=False)
    assert r.returncode != 0 and "(ERROR)" in r.stderr, r.stderr[-500:]
    # an archive without qualities decompressed without -Q
    open(tmp_path / "q_1.fq", "wb").write(fq)
    run("-Q", "-c", "no", "-o", tmp_path / "q", tmp_path / "q_1.fq", "--patterns-bin", F.PBIN)
    r = run("-d", "-o", tmp_path / "qback", tmp_path / "q_1.scalcen", "--patterns-bin", F.PBIN, ok=False)
    assert r.returncode != 0 and "(ERROR)" in r.stderr and "-Q" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(tmp_path / "qback_1.fastq")
    # one GPU only
    for mode in ("-f", "-Q"):
        r = run(mode, "--gpus", "2", "-c", "no", "-o", tmp_path / "g", tmp_path / "q_1.fq", "--patterns-bin", F.PBIN, ok=False)
        assert r.returncode != 0 and "(ERROR)" in r.stderr, r.stderr[-500:]
