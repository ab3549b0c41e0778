"""-m gpu: `scalce --keep-comments` and the comments put back by `scalce -d`, as a program.

Round trip: --keep-order --keep-comments, then -d, gives the input file byte for byte.  Without --keep-order, -d is the
-d --no-comments text with comment_ref's entries put in.  Every other file of the archive is the one the run without the
option writes, and the reference's own decompress() reads the archive.  Then windows, ranges, -S, -o -, the device memory of
a small window, a stale stream, damaged streams and refusals."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import comment_ref as CR
import filecases as F
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
have_ref = pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")
N, L = 3000, 60


def scalce(*args, ok=True):
    r = subprocess.run([F.SCALCE, *map(str, args), "--patterns-bin", F.PBIN], capture_output=True, timeout=600)
    if ok is not None:
        assert (r.returncode == 0) == ok, (args, r.returncode, r.stderr[-1500:])
    return r


def read(p):
    return open(p, "rb").read()


def write(p, data):
    with open(p, "wb") as f:
        f.write(data)
    return str(p)


def cut(text, lines):
    ls = text.split(b"\n")
    assert ls[-1] == b"" and (len(ls) - 1) % lines == 0, (len(ls), lines)
    return [b"\n".join(ls[i:i + lines]) + b"\n" for i in range(0, len(ls) - 1, lines)]


def header(r, mate, slash):
    """Illumina-style and SRA-style header lines, some without a comment, one that ends in a space.  Both mates of a pair
    share the name (or differ in /1 and /2 alone, as -d restores it)."""
    kind = r % 5
    tail = (b"/%d" % mate) if slash else b""
    if kind == 0:
        return b"M01:23:000-A1:1:1101:%d:%d" % (1000 + r, 2000 + 7 * r) + tail + b" %d:N:0:ATCACG+%04d" % (mate, r % 97)
    if kind == 1:
        return b"SRR100.%d" % r + tail + b" HWI-ST745:%d:%d length=%d" % (r, mate, L)
    if kind == 2:
        return b"plain.%d" % r + tail
    if kind == 3:
        return b"sp.%d" % r + tail + b" "
    return b"t\tab.%d" % r + tail + b"  two  spaces %d" % mate


def fastq(n, length, seed, mate=1, slash=False, lens=None, fasta=False):
    bases, quals = synth.reads_and_quals(n, length, seed=seed, dup_frac=0.2)
    out = []
    for r in range(n):
        k = length if lens is None else int(lens[r])
        b, q = bases[r, :k].tobytes(), quals[r, :k].tobytes()
        h = header(r, mate, slash)
        # (two-line records come back with '@' in front of the name, whatever the input had: the FASTA case writes '@' itself)
        out.append(b"@" + h + b"\n" + b + b"\n" if fasta else b"@" + h + b"\n" + b + b"\n+\n" + q + b"\n")
    return b"".join(out)


def interleaved(a, b):
    return b"".join(x + y for x, y in zip(cut(a, 4), cut(b, 4)))


# name -> compress flags, decompress flags, lines per record of the output, files written by -d
CASES = {
    "se": dict(c=[], d=[], lines=4, mates=1),
    "pe": dict(c=["-r"], d=["-r"], lines=4, mates=2),
    "il": dict(c=["-i"], d=["-i"], lines=8, mates=1),
    "f": dict(c=["-f"], d=["-f"], lines=2, mates=1),
    "varlen": dict(c=["--variable-length"], d=[], lines=4, mates=1),
    "gz": dict(c=["-c", "gz"], d=[], lines=4, mates=1),
    "no": dict(c=["-c", "no"], d=[], lines=4, mates=1),
    "gzin": dict(c=[], d=[], lines=4, mates=1),
    "two": dict(c=[], d=[], lines=4, mates=1),
}


class Case:
    """a case's input and its archives: plain, --keep-comments, and --keep-order --keep-comments"""

    def __init__(self, name, root):
        self.name, self.c = name, CASES[name]
        self.d = d = str(root.mktemp("kc_" + name))
        ins = [os.path.join(d, "in_1.fq")]
        if name == "pe":
            self.input = [fastq(N, L, 31, 1, True), fastq(N, L, 32, 2, True)]
            write(ins[0], self.input[0])
            write(os.path.join(d, "in_2.fq"), self.input[1])
        elif name == "il":
            self.mates_text = [fastq(N, L, 31, 1, True), fastq(N, L, 32, 2, True)]
            self.input = [interleaved(*self.mates_text)]
            write(ins[0], self.input[0])
        elif name == "f":
            self.input = [fastq(N, L, 33, fasta=True)]
            write(ins[0], self.input[0])
        elif name == "varlen":
            lens = np.random.default_rng(34).integers(0, L + 1, size=N)
            lens[:L + 1] = np.arange(L + 1)
            self.input = [fastq(N, L, 35, lens=lens)]
            write(ins[0], self.input[0])
        elif name == "gzin":
            self.input = [fastq(N, L, 36)]
            ins = [os.path.join(d, "in_1.fq.gz")]
            write(ins[0], gzip.compress(self.input[0], 1))
        elif name == "two":
            self.input = [fastq(N, L, 37)]
            recs = cut(self.input[0], 4)
            ins = [os.path.join(d, "ina_1.fq"), os.path.join(d, "inb_1.fq")]
            write(ins[0], b"".join(recs[:1100]))
            write(ins[1], b"".join(recs[1100:]))
        else:
            self.input = [fastq(N, L, 30 + len(name))]
            write(ins[0], self.input[0])
        self.ins = ins
        self.common = ["-s", "1000"] + ([] if "-c" in self.c["c"] else ["-c", "no"])
        self.logs = {}
        for out, flags in (("plain", []), ("com", ["--keep-comments"]), ("both", ["--keep-order", "--keep-comments"])):
            self.logs[out] = scalce(*self.c["c"], *self.common, *flags, "-o", os.path.join(d, out), *ins).stderr.decode()
        self.files = 2 if name in ("pe", "il") else 1    # mates the archive holds

    def arc(self, which):
        return os.path.join(self.d, which + "_1.scalcen")

    def decompress(self, which, out, *flags, ok=True):
        return scalce("-d", *self.c["d"], "-o", os.path.join(self.d, out) if out != "-" else "-", self.arc(which), *flags, ok=ok)

    def outputs(self, out):
        return [read(os.path.join(self.d, "%s_%d.fastq" % (out, m + 1))) for m in range(self.c["mates"])]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory)
        return made[name]
    return get


# ---- round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_keep_order_and_keep_comments_return_the_input(name, cases):
    k = cases(name)
    k.decompress("both", "rt")
    assert k.outputs("rt") == k.input


@pytest.mark.parametrize("name", ["se", "pe", "f", "varlen"])
def test_without_keep_order_the_entries_go_into_the_plain_text(name, cases):
    k = cases(name)
    k.decompress("com", "nc", "--no-comments")
    k.decompress("plain", "pl")
    k.decompress("com", "wc")
    bare = k.outputs("nc")
    assert bare == k.outputs("pl")   # --no-comments: what -d writes today
    lines = k.c["lines"]
    for m, text in enumerate(k.outputs("wc")):
        ents = host.unpack_comments(F.content(os.path.join(k.d, "com_%d.scalcec" % (m + 1))))
        recs = cut(bare[m], lines)
        want, _ = CR.insert(bare[m], np.cumsum([0] + [len(r) for r in recs]), ents, lines_per_record=lines)
        assert text == want
        # ... and they are the input's entries, each with the record it came with
        by_record = {r.split(b"\n", 1)[1]: CR.entry_of(r.split(b"\n")[0]) for r in cut(k.input[m], lines)}
        if len(by_record) == N:   # (no two records share bases and qualities)
            assert all(CR.entry_of(r.split(b"\n")[0]) == by_record[r.split(b"\n", 1)[1]] for r in cut(text, lines))


def test_ignoring_names_ignores_the_comments(cases):
    k = cases("se")
    k.decompress("com", "nn", "-n", "lib")
    k.decompress("plain", "pn", "-n", "lib")
    assert k.outputs("nn") == k.outputs("pn")


# ---- the other files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_other_file_is_the_one_without_the_option(name, cases):
    k = cases(name)
    exts = "rnq" + ("l" if name == "varlen" else "")
    for m in range(k.files):
        for e in exts:
            a, b = (os.path.join(k.d, "%s_%d.scalce%s" % (w, m + 1, e)) for w in ("plain", "com"))
            assert read(a) == read(b), (m, e)
            assert read(a) == read(os.path.join(k.d, "both_%d.scalce%s" % (m + 1, e))), (m, e)
        assert not os.path.exists(os.path.join(k.d, "plain_%d.scalcec" % (m + 1)))
        data = F.content(os.path.join(k.d, "com_%d.scalcec" % (m + 1)))
        assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24])[0] == 0 and struct.unpack("<iiq", data[8:24])[2] == N
        raw = read(os.path.join(k.d, "com_%d.scalcec" % (m + 1)))
        assert (raw[:2] == b"\x1f\x8b") == (name == "gz")
    # the log: one line per mate, and none without the option
    got = re.findall(r"Comments: (\d+) records, (\d+) bytes, longest (\d+)", k.logs["com"])
    assert len(got) == k.files and "Comments:" not in k.logs["plain"]
    for m, (n, nbytes, longest) in enumerate(got):
        data = F.content(os.path.join(k.d, "com_%d.scalcec" % (m + 1)))
        assert (int(n), int(nbytes), int(longest)) == (N, len(data) - 24, struct.unpack("<iiq", data[8:24])[1])


def test_the_stream_holds_the_inputs_entries_in_archive_order(cases):
    for name in ("se", "pe", "il"):
        k = cases(name)
        perm = host.unpack_order(F.content(os.path.join(k.d, "both_1.scalceo")))
        texts = k.mates_text if name == "il" else k.input
        for m, text in enumerate(texts):
            ents = CR.entries(text)[0]
            assert F.content(os.path.join(k.d, "both_%d.scalcec" % (m + 1))) == CR.stream(ents, perm), (name, m)


@have_ref
def test_the_reference_reads_the_archive(cases, tmp_path):
    k = cases("se")
    r = subprocess.run([F.REF_FULL, "decompress", F.PBIN, k.arc("com"), str(tmp_path / "back"), "-T", "1"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    k.decompress("com", "nc2", "--no-comments")
    assert read(tmp_path / "back_1.fastq") == k.outputs("nc2")[0]


# ---- windows and ranges -------------------------------------------------------------------------------------------------------
REC = 2 * L + 6 + 60   # about a record with its name and its entry


@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen"])
@pytest.mark.parametrize("window", [1, REC * 7, REC * 400], ids=["one_record", "a_few_records", "eight_windows"])
def test_windows_of_every_size_give_the_same_text(window, name, cases):
    k = cases(name)
    k.decompress("com", "w0")
    k.decompress("com", "w%d" % window, "--window", window)
    assert k.outputs("w%d" % window) == k.outputs("w0")
    k.decompress("both", "wo%d" % window, "--window", window)
    assert k.outputs("wo%d" % window) == k.input


def test_record_ranges_concatenate_to_the_whole(cases):
    k = cases("se")
    k.decompress("com", "all")
    whole = k.outputs("all")[0]
    recs = cut(whole, 4)
    slices = []
    for first, count in ((0, 1), (1, 699), (700, 1), (701, 1500), (2201, N)):
        k.decompress("com", "rg%d" % first, "--records", "%d:%d" % (first, count), "--window", REC * 300)
        slices.append(k.outputs("rg%d" % first)[0])
        assert slices[-1] == b"".join(recs[first:first + count])
    assert b"".join(slices) == whole
    k.decompress("com", "rgend", "--records", str(N))
    assert k.outputs("rgend")[0] == b""
    k.decompress("both", "rgao", "--records", "10:5", "--archive-order")
    assert k.outputs("rgao")[0] == b"".join(recs[10:15])


def test_split_parts_and_stdout(cases):
    k = cases("se")
    per = 700
    k.decompress("both", "sp", "-S", per, "--window", REC * 300)
    parts = [read(os.path.join(k.d, "sp.%d_1.fastq" % (i + 1))) for i in range((N + per - 1) // per)]
    assert b"".join(parts) == k.input[0] and [len(cut(p, 4)) for p in parts] == [700, 700, 700, 700, 200]
    r = k.decompress("both", "-", "--window", REC * 500)
    assert r.stdout == k.input[0]
    k.decompress("com", "wc0")
    r = k.decompress("com", "-", "--window", REC * 500)
    assert r.stdout == k.outputs("wc0")[0]


def held(r):
    return int(re.search(r"device memory held at most (\d+) bytes", r.stderr.decode()).group(1))


def test_device_memory_follows_the_window(cases):
    """a small window with comments holds what the same run holds without them, plus -- per slot -- the window's entries, the
    text with them put back, its offsets and the insert pass's scratch, all sized by the window's records R and the header's C"""
    k = cases("se")
    window = REC * 100
    with_c = held(k.decompress("com", "m1", "--window", window))
    without = held(k.decompress("com", "m0", "--window", window, "--no-comments"))
    whole = held(k.decompress("com", "m2"))
    C = struct.unpack("<iiq", F.content(os.path.join(k.d, "com_1.scalcec"))[8:24])[1]
    R = window // (2 * L + 6)
    per_slot = (R * (C + 1) + 64) + (max(window, 2 * L + 6 + 255 + 32 + C) + 64 + C) + 2 * 8 * (R + 1) + host.fastq_comment_ws_bytes(R, R * (C + 1) + 64) + 64
    assert without < with_c <= without + 2 * (per_slot + 6 * 256) + 2 * C
    assert with_c < whole   # of the window's order: the default window holds the whole archive and is sized for far more


# ---- a stale stream -----------------------------------------------------------------------------------------------------------
def test_a_later_run_without_the_option_removes_the_stream(cases, tmp_path):
    k = cases("pe")
    out = tmp_path / "x"
    scalce("-r", *k.common, "--keep-comments", "-o", out, *k.ins)
    assert os.path.exists(tmp_path / "x_1.scalcec") and os.path.exists(tmp_path / "x_2.scalcec")
    scalce("-r", *k.common, "-o", out, *k.ins)
    assert not os.path.exists(tmp_path / "x_1.scalcec") and not os.path.exists(tmp_path / "x_2.scalcec")


# ---- errors -------------------------------------------------------------------------------------------------------------------
def damaged(k, tmp_path, change):
    for ext in "rnqc":
        data = read(os.path.join(k.d, "com_1.scalce%s" % ext))
        write(tmp_path / ("a_1.scalce%s" % ext), change(data) if ext == "c" else data)
    return tmp_path / "a_1.scalcen"


def fails_with(arc, tmp_path, word, *flags):
    r = scalce("-d", "-o", tmp_path / "out", arc, *flags, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and word in err, err[-800:]


def test_damaged_streams(cases, tmp_path):
    k = cases("se")
    data = read(os.path.join(k.d, "com_1.scalcec"))
    ends = [i for i in range(24, len(data)) if data[i] == 10]
    inside = next(e for e in ends[100:] if data[e - 1] != 10) - 3   # inside an entry
    for i, (change, word) in enumerate([
            (lambda d: d[:inside], "truncated comment stream"),
            (lambda d: d[:ends[1500] + 1], "truncated comment stream"),                 # between two entries
            (lambda d: d[:20], "truncated comment stream"),
            (lambda d: b"notscalc" + d[8:], "is not a scalce comment stream"),
            (lambda d: d[:8] + struct.pack("<i", 4) + d[12:], "is not a scalce comment stream"),
            (lambda d: d[:16] + struct.pack("<q", N - 1) + d[24:], "comment stream holds %d entries, the archive %d records" % (N - 1, N)),
            (lambda d: d[:16] + struct.pack("<q", N + 1) + d[24:], "comment stream holds %d entries, the archive %d records" % (N + 1, N)),
            (lambda d: d[:12] + struct.pack("<i", 3) + d[16:], "comment stream: an entry is longer than its header says")]):
        sub = tmp_path / ("case%d" % i)
        os.mkdir(sub)
        fails_with(damaged(k, sub, change), sub, word, "--window", REC * 200)


def test_refusals(cases, tmp_path):
    k = cases("se")
    for flags, word in ((["--keep-comments", "-n", "lib"], "-n"), (["--keep-comments", "--gpus", "2", "-B", "1M"], "--gpus"),
                        (["--keep-comments", "-d"], "--keep-comments"), (["--no-comments"], "--no-comments")):
        src = k.arc("com") if "-d" in flags else k.ins[0]
        r = scalce(*flags, "-c", "no", "-o", tmp_path / "x", src, ok=False)
        err = r.stderr.decode()
        assert r.returncode == 1 and "(ERROR)" in err and word in err, err
        assert os.listdir(tmp_path) == []
    r = scalce("--keep-comments", "-n", "lib", "-o", tmp_path / "x", k.ins[0], ok=False)
    assert "nothing is kept for what follows a name that is not kept" in r.stderr.decode()
