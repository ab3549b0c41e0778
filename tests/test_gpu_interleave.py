"""Interleaved paired-end FASTQ (-i): one file, mate 1 then mate 2 of every pair, compressed and decompressed on the device.

The contract: the -i archive of an interleaved file is byte for byte the -r archive of the same pairs split into _1 / _2
files.  The -r archive is pinned to the reference by the file-case tests; where oracle/_ref/ref_full is built, the -i
archive is compared with the reference's own -r archive of the split pair as well.  -d -i writes the records -d -r writes,
interleaved again.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import filecases as F
from scalce_amd import synth

pytestmark = pytest.mark.gpu

PBIN = F.PBIN


def run(*args, ok=True, env=None):
    r = subprocess.run([F.SCALCE, *map(str, args)], capture_output=True, env=env, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def records(n, L, seed, mate, fasta=False):
    """one mate's records as a list of bytes: '@p.<i>/<mate>' names (no comment), a bare '+' line, and '!' under every N (the
    quality an N is stored with, qualities.cpp:183): records -d restores byte for byte"""
    bases, quals = synth.reads_and_quals(n, L, seed=seed, dup_frac=0.1, n_frac=0.005)
    quals = np.where(bases == ord("N"), ord("!"), quals).astype(np.uint8)
    if fasta:
        return [b">p.%d/%d\n" % (i, mate) + bases[i].tobytes() + b"\n" for i in range(n)]
    return [b"@p.%d/%d\n" % (i, mate) + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i in range(n)]


def pairs(n, L1=100, L2=None, seed=7, fasta=False):
    return records(n, L1, seed, 1, fasta), records(n, L2 or L1, seed + 1, 2, fasta)


def interleave(r1, r2):
    return b"".join(a + b for a, b in zip(r1, r2))


def fastq_records(text, lpr=4):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % lpr == 0
    return [b"\n".join(lines[i:i + lpr]) + b"\n" for i in range(0, len(lines) - 1, lpr)]


def pair_set(text, lpr=4):
    """the pairs of an interleaved text, sorted: the archive holds them in bucket order, not in input order"""
    recs = fastq_records(text, lpr)
    assert len(recs) % 2 == 0
    return sorted(recs[i] + recs[i + 1] for i in range(0, len(recs), 2))


def write_case(d, r1, r2, tag="in"):
    """the interleaved file and the split pair; returns (interleaved path, mate-1 path of the split pair)"""
    il, s1, s2 = d / f"{tag}_il.fq", d / f"{tag}_split_1.fq", d / f"{tag}_split_2.fq"
    il.write_bytes(interleave(r1, r2))
    s1.write_bytes(b"".join(r1))
    s2.write_bytes(b"".join(r2))
    return il, s1


def cli_flags(flags):
    """ref_full spelling (-B in bytes) -> the CLI's (-B in M)"""
    out = list(flags)
    if "-B" in out:
        i = out.index("-B")
        out[i + 1] = "%dM" % (int(out[i + 1]) >> 20)
    return out


def archive(d, prefix):
    return {(m, ext): F.content(d / f"{prefix}_{m}.scalce{ext}") for m in (1, 2) for ext in "nrq"}


def assert_same_archive(d, a, b, what):
    A, B = archive(d, a), archive(d, b)
    for k in A:
        assert A[k] == B[k], f"{what}: mate {k[0]} .scalce{k[1]} differs ({len(A[k])} vs {len(B[k])} bytes)"


def compress_both(d, il_inputs, split_inputs, flags, env=None):
    """scalce -i on the interleaved input(s) and scalce -r on the split pair(s), -c no; the reference's -r where it is built
    (the reference harness takes no -Q / -f: those archives are pinned through -r by tests/test_gpu_no_qualities.py)"""
    ins = [il_inputs] if not isinstance(il_inputs, list) else il_inputs
    sins = [split_inputs] if not isinstance(split_inputs, list) else split_inputs
    run("-i", *cli_flags(flags), "-c", "no", "-o", d / "il", *ins, "--patterns-bin", PBIN, env=env)
    for m in (1, 2):
        for ext in "nrq":
            assert (d / f"il_{m}.scalce{ext}").exists(), f"-i wrote no il_{m}.scalce{ext}"
    run("-r", *cli_flags(flags), "-c", "no", "-o", d / "rr", *sins, "--patterns-bin", PBIN)
    assert_same_archive(d, "il", "rr", "-i vs -r of the split pair")
    if os.path.exists(F.REF_FULL) and "-Q" not in flags and "-f" not in flags:
        subprocess.run([F.REF_FULL, "compress", PBIN, ",".join(map(str, sins)), str(d / "ref"), "-r", *flags, "-T", "1",
                        "-t", str(d / "tmp_ref")], check=True, capture_output=True, timeout=600)
        assert_same_archive(d, "il", "ref", "-i vs the reference's -r of the split pair")


def decompress_both(d, extra=()):
    """-d -i of the -i archive, and -d -r of the -r archive interleaved here: both texts"""
    run("-d", "-i", *extra, "-o", d / "back", d / "il_1.scalcen", "--patterns-bin", PBIN)
    run("-d", "-r", *extra, "-o", d / "rback", d / "rr_1.scalcen", "--patterns-bin", PBIN)
    assert not (d / "back_2.fastq").exists(), "-d -i writes ONE file"
    lpr = 2 if ("-Q" in extra or "-f" in extra) else 4
    got = (d / "back_1.fastq").read_bytes()
    want = interleave(fastq_records((d / "rback_1.fastq").read_bytes(), lpr), fastq_records((d / "rback_2.fastq").read_bytes(), lpr))
    assert got == want, "-d -i is not -d -r interleaved"
    return got


# ---- archive identity, and the round trip of each archive ------------------------------------------------------------
FLAG_SETS = {
    "default": ([], dict(n=6000)),
    "nlib": (["-n", "lib"], dict(n=6000)),
    "A": (["-A"], dict(n=6000)),
    "p30": (["-p", "30"], dict(n=6000)),
    "B": (["-B", "1048576"], dict(n=14000)),            # several spill chunks
    "mixed_len": ([], dict(n=6000, L1=100, L2=150)),
    "long": ([], dict(n=1500, L1=300, L2=270)),          # two-byte end marker (reads.cpp:106-108), indexed ingest
    "short": ([], dict(n=4000, L1=12, L2=40)),           # below the tile kernel: indexed ingest for mate 1
}


@pytest.mark.parametrize("case", sorted(FLAG_SETS))
def test_archive_is_the_split_pairs_archive(case, tmp_path):
    flags, shape = FLAG_SETS[case]
    r1, r2 = pairs(shape["n"], shape.get("L1", 100), shape.get("L2"), seed=11)
    il, s1 = write_case(tmp_path, r1, r2)
    compress_both(tmp_path, il, s1, flags)
    got = decompress_both(tmp_path)  # (-n: the library name comes from the archive)
    if "-n" not in flags and "-p" not in flags:  # canonical records, lossless qualities: the input's pairs come back
        assert pair_set(got) == pair_set(il.read_bytes()), f"{case}: -d -i did not restore the interleaved input's pairs"


@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_archive_without_qualities(mode, tmp_path):
    r1, r2 = pairs(5000, 100, 120, seed=13, fasta=mode == "-f")
    il, s1 = write_case(tmp_path, r1, r2)
    compress_both(tmp_path, il, s1, [mode])
    got = decompress_both(tmp_path, ("-Q",))
    if mode == "-Q":  # two-line records: name and bases (an N, stored as a 0 base, comes back as A)
        want = [rec.split(b"\n")[:2] for rec in fastq_records(il.read_bytes())]
        assert pair_set(got, 2) == pair_set(b"".join(a + b"\n" + b.replace(b"N", b"A") + b"\n" for a, b in want), 2)


# ---- input shapes ---------------------------------------------------------------------------------------------------
def test_gzip_input(tmp_path):
    r1, r2 = pairs(5000, seed=17)
    il, s1 = write_case(tmp_path, r1, r2)
    gz = tmp_path / "in_il.fq.gz"
    gz.write_bytes(gzip.compress(il.read_bytes(), 1))
    compress_both(tmp_path, gz, s1, [])


def test_several_input_files(tmp_path):
    """three files, each of whole pairs (the first shorter than -s); the -r run takes the same three split pairs"""
    r1, r2 = pairs(9000, 100, 110, seed=19)
    cuts = [0, 700, 5100, 9000]
    ils, splits = [], []
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        il, s1 = write_case(tmp_path, r1[a:b], r2[a:b], tag="part%c" % (97 + k))
        ils.append(il)
        splits.append(s1)
    compress_both(tmp_path, ils, splits, ["-s", "2000", "-p", "30"])


def test_streamed_in_pieces(tmp_path):
    """pieces of a size no pair divides: every piece ends on a pair boundary, the rest opens the next one"""
    r1, r2 = pairs(12000, 100, 130, seed=23)
    il, s1 = write_case(tmp_path, r1, r2)
    env = dict(os.environ, SCALCE_PIECE_BYTES="300007")
    run("-i", "-B", "1M", "-c", "no", "-o", tmp_path / "il", il, "--patterns-bin", PBIN, env=env)
    run("-r", "-B", "1M", "-c", "no", "-o", tmp_path / "rr", s1, "--patterns-bin", PBIN)
    assert_same_archive(tmp_path, "il", "rr", "-i in pieces vs -r")


def test_last_record_without_newline(tmp_path):
    r1, r2 = pairs(3000, seed=29)
    il, s1 = write_case(tmp_path, r1, r2)
    il.write_bytes(il.read_bytes()[:-1])
    compress_both(tmp_path, il, s1, [])


# ---- decompression: -S, stdout ----------------------------------------------------------------------------------------
def test_split_parts_and_stdout(tmp_path):
    r1, r2 = pairs(10, seed=31)
    il, s1 = write_case(tmp_path, r1, r2)
    compress_both(tmp_path, il, s1, [])
    text = decompress_both(tmp_path)
    assert pair_set(text) == pair_set(il.read_bytes())
    run("-d", "-i", "-S", "3", "-o", tmp_path / "part", tmp_path / "il_1.scalcen", "--patterns-bin", PBIN)
    parts = [(tmp_path / f"part.{k}_1.fastq").read_bytes() for k in (1, 2, 3, 4)]
    assert not (tmp_path / "part.5_1.fastq").exists() and not (tmp_path / "part.1_2.fastq").exists()
    recs = fastq_records(text)
    for k, p in enumerate(parts):
        assert p == b"".join(recs[6 * k:6 * k + 6]), f"part {k + 1} does not hold pairs {3 * k} .. {3 * k + 2} of -d -i's text"
    r = run("-d", "-i", "-o", "-", tmp_path / "il_1.scalcen", "--patterns-bin", PBIN)
    assert r.stdout == text


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors(tmp_path):
    r1, r2 = pairs(400, seed=37)
    il, s1 = write_case(tmp_path, r1, r2)
    r = run("-i", "-r", "-c", "no", "-o", tmp_path / "e1", s1, "--patterns-bin", PBIN, ok=False)
    assert r.returncode != 0 and b"Interleaved option (-i) cannot be used with paired-end option (-r)" in r.stderr
    r = run("-i", "--gpus", "2", "-c", "no", "-o", tmp_path / "e2", il, "--patterns-bin", PBIN, ok=False)
    assert r.returncode != 0 and b"-i runs on one GPU" in r.stderr, r.stderr[-400:]
    odd = tmp_path / "odd.fq"
    odd.write_bytes(interleave(r1, r2) + r1[0])
    r = run("-i", "-c", "no", "-o", tmp_path / "e3", odd, "--patterns-bin", PBIN, ok=False)
    assert r.returncode != 0 and b"odd number of records" in r.stderr and str(odd).encode() in r.stderr, r.stderr[-400:]
    # an odd file in front of an even one: the pairs would shift, so the file is named even though the total is even
    r = run("-i", "-c", "no", "-o", tmp_path / "e4", odd, odd, "--patterns-bin", PBIN, ok=False)
    assert r.returncode != 0 and b"odd number of records" in r.stderr and str(odd).encode() in r.stderr, r.stderr[-400:]
    for e in ("e1", "e2", "e3", "e4"):
        assert not list(tmp_path.glob(e + "_*")), f"{e}: an archive was left behind"


# ---- the batch API ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L1,L2", [(100, 100), (90, 140), (200, 180)])
def test_batch_interleaved_equals_two_texts(L1, L2):
    import torch

    from gpu_util import device_bytes
    from scalce_amd import host

    n = 5000
    r1, r2 = pairs(n, L1, L2, seed=41)
    t1, t2, ti = b"".join(r1), b"".join(r2), interleave(r1, r2)
    ctx = host.Context(0, patterns_bin=open(PBIN, "rb").read())
    qm = [(33, list(range(128))), (33, list(range(128)))]
    d1, d2, di = device_bytes(t1), device_bytes(t2), device_bytes(ti)
    two = host.Batch(ctx, L1, n + 8, max(len(t1), len(t2)) + 64, paired=True, read_len2=L2, qmap=qm, bucket_set_size=1 << 20)
    two.compress(d1.data_ptr(), len(t1), d2.data_ptr(), len(t2))
    two.finish()
    one = host.Batch(ctx, L1, n + 8, len(ti) + 64, paired=True, read_len2=L2, qmap=qm, bucket_set_size=1 << 20, interleaved=True)
    one.compress(di.data_ptr(), len(ti))
    one.finish()
    torch.cuda.synchronize()
    assert one.n_reads == two.n_reads == n
    for which, dt in ((host.OUT_TOKENS, np.int32), (host.OUT_PERM, np.uint32)):
        assert np.array_equal(one.output(which, 0, dt), two.output(which, 0, dt)), f"output {which}"
    for m in (0, 1):
        for which in (host.OUT_READS, host.OUT_QINPUT, host.OUT_QUAL):
            a, b = one.output(which, m), two.output(which, m)
            assert len(a) == len(b) and np.array_equal(a, b), f"mate {m + 1} output {which}"
    assert np.array_equal(one.output(host.OUT_NAMES, 0), two.output(host.OUT_NAMES, 0))
    # appended in pieces of whole pairs: the same rows
    app = host.Batch(ctx, L1, n + 8, len(ti) + 64, paired=True, read_len2=L2, qmap=qm, bucket_set_size=1 << 20, interleaved=True)
    cut = len(b"".join(a + b for a, b in zip(r1[:1234], r2[:1234]))) + 17  # inside pair 1234
    u0, u1 = app.append(di.data_ptr(), cut)
    assert u1 == 0 and u0 == cut - 17, (u0, u1)
    rest = device_bytes(ti[u0:])
    app.append(rest.data_ptr(), len(ti) - u0, final=True)
    app.order(); app.emit(); app.entropy(); app.finish()
    assert app.n_reads == n
    for m in (0, 1):
        assert np.array_equal(app.output(host.OUT_READS, m), two.output(host.OUT_READS, m)), f"appended: mate {m + 1} reads"
        assert np.array_equal(app.output(host.OUT_QUAL, m), two.output(host.OUT_QUAL, m)), f"appended: mate {m + 1} qualities"
    with pytest.raises(host.ScalceError):
        one.ingest(1, di.data_ptr(), len(ti))
    odd = device_bytes(ti + r1[0])
    with pytest.raises(host.ScalceError, match="odd number of records"):
        one.ingest(0, odd.data_ptr(), len(ti) + len(r1[0]))
