"""-m gpu: `scalce --keep-plus`, `--lossless` and the '+' lines put back by `scalce -d`, as a program.

Round trip: --lossless, then -d, gives the input file byte for byte -- SRA-style headers repeated on the third line, lower-case
and IUPAC letters, N under a quality other than the lowest.  --keep-plus alone: -d is the -d --bare-plus text with plus_ref's
entries put in.  Every other file of the archive is the one the run without the option writes, and the reference's own
decompress() reads the archive.  Then windows, ranges, -S, a stale stream, damaged streams and refusals."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import filecases as F
import plus_ref as PR
from scalce_amd import format as fmt
from scalce_amd import synth

pytestmark = pytest.mark.gpu
have_ref = pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")
N, L = 3000, 60
REC = 2 * (2 * L + 6 + 60)   # about a record with its header line on both lines


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


def cut(text, lines=4):
    ls = text.split(b"\n")
    assert ls[-1] == b"" and (len(ls) - 1) % lines == 0, (len(ls), lines)
    return [b"\n".join(ls[i:i + lines]) + b"\n" for i in range(0, len(ls) - 1, lines)]


def header(r, mate, slash, length):
    """fastq-dump style, some without a comment; both mates of a pair share the name (or differ in /1 and /2 alone)"""
    tail = (b"/%d" % mate) if slash else b""
    if r % 5 == 4:
        return b"plain.%d" % r + tail
    return b"SRR001666.%d" % r + tail + b" 071112_SLXA-EAS1_s_7:5:1:%d:%d length=%d" % (817 + r % 13, 345 + r, length)


def third(r, head):
    kind = r % 7
    if kind in (0, 1, 2, 3):
        return b"+" + head                     # the header again, as fastq-dump writes it
    if kind == 4:
        return b"+"
    if kind == 5:
        return b"+" + head.split(b" ")[0]      # the name alone
    return (b"+=", b"+'quoted'", b"+ ")[r % 3]


def fastq(n, length, seed, mate=1, slash=False, lens=None):
    bases, quals = synth.reads_and_quals(n, length, seed=seed, dup_frac=0.2, n_frac=0.01)
    rng = np.random.default_rng(seed + 1000)
    odd = np.frombuffer(b"acgtnRYKMSWBDHVN", dtype=np.uint8)   # lower case, IUPAC codes, and N under whatever quality is there
    where = rng.random(bases.shape) < 0.02
    bases = np.where(where, odd[rng.integers(0, len(odd), size=bases.shape)], bases).astype(np.uint8)
    out = []
    for r in range(n):
        k = length if lens is None else int(lens[r])
        h = header(r, mate, slash, k)
        out.append(b"@" + h + b"\n" + bases[r, :k].tobytes() + b"\n" + third(r, h) + b"\n" + quals[r, :k].tobytes() + b"\n")
    return b"".join(out)


def interleaved(a, b):
    return b"".join(x + y for x, y in zip(cut(a), cut(b)))


# name -> compress flags, decompress flags, files written by -d
CASES = {
    "se": dict(c=[], d=[], mates=1),
    "pe": dict(c=["-r"], d=["-r"], mates=2),
    "il": dict(c=["-i"], d=["-i"], mates=1),
    "varlen": dict(c=["--variable-length"], d=[], mates=1),
    "gz": dict(c=["-c", "gz"], d=[], mates=1),
    "B": dict(c=["-B", "1M"], d=[], mates=1, n=20000),
    "gzin": dict(c=[], d=[], mates=1),
    "two": dict(c=[], d=[], mates=1),
}


class Case:
    """a case's input and its archives: plain, --keep-plus and --lossless"""

    def __init__(self, name, root):
        self.name, self.c = name, CASES[name]
        self.n = n = self.c.get("n", N)
        self.d = d = str(root.mktemp("kp_" + name))
        ins = [os.path.join(d, "in_1.fq")]
        if name == "pe":
            self.input = [fastq(n, L, 31, 1, True), fastq(n, L, 32, 2, True)]
            write(ins[0], self.input[0])
            write(os.path.join(d, "in_2.fq"), self.input[1])
        elif name == "il":
            self.mates_text = [fastq(n, L, 31, 1, True), fastq(n, L, 32, 2, True)]
            self.input = [interleaved(*self.mates_text)]
            write(ins[0], self.input[0])
        elif name == "varlen":
            lens = np.random.default_rng(34).integers(0, L + 1, size=n)
            lens[:L + 1] = np.arange(L + 1)
            self.input = [fastq(n, L, 35, lens=lens)]
            write(ins[0], self.input[0])
        elif name == "gzin":
            self.input = [fastq(n, L, 36)]
            ins = [os.path.join(d, "in_1.fq.gz")]
            write(ins[0], gzip.compress(self.input[0], 1))
        elif name == "two":
            self.input = [fastq(n, L, 37)]
            recs = cut(self.input[0])
            ins = [os.path.join(d, "ina_1.fq"), os.path.join(d, "inb_1.fq")]
            write(ins[0], b"".join(recs[:1100]))
            write(ins[1], b"".join(recs[1100:]))
        else:
            self.input = [fastq(n, L, 30 + len(name))]
            write(ins[0], self.input[0])
        self.ins = ins
        self.common = ["-s", "1000"] + ([] if "-c" in self.c["c"] else ["-c", "no"])
        self.logs = {}
        for out, flags in (("plain", []), ("plus", ["--keep-plus"]), ("all", ["--lossless"])):
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


# ---- the lossless round trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lossless_returns_the_input(name, cases):
    k = cases(name)
    k.decompress("all", "rt")
    assert k.outputs("rt") == k.input
    if name == "B":   # the run was cut into spill chunks
        assert int(re.search(r"Spill chunks: (\d+)", k.logs["all"]).group(1)) >= 2, k.logs["all"]


def test_the_input_holds_what_only_lossless_brings_back(cases):
    k = cases("se")
    text = k.input[0]
    recs = cut(text)
    assert sum(r.split(b"\n")[2] == b"+" + r.split(b"\n")[0][1:] and len(r.split(b"\n")[2]) > 1 for r in recs) > N // 2
    seqs = b"".join(r.split(b"\n")[1] for r in recs)
    assert any(c in seqs for c in b"acgt") and any(c in seqs for c in b"RYKMSW")
    assert any(q != min(r.split(b"\n")[3]) for r in recs for b, q in zip(r.split(b"\n")[1], r.split(b"\n")[3]) if b == ord("N"))
    k.decompress("plain", "pl")
    assert k.outputs("pl") != k.input


@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen"])
@pytest.mark.parametrize("window", [1, REC * 7, REC * 400], ids=["one_record", "a_few_KiB", "several_windows"])
def test_lossless_through_windows_of_every_size(window, name, cases):
    k = cases(name)
    r = k.decompress("all", "w%d" % window, "--window", window)
    assert k.outputs("w%d" % window) == k.input
    if window == 1:
        assert int(re.search(r"Windows: (\d+)", r.stderr.decode()).group(1)) >= N


def test_lossless_split_parts_and_stdout(cases):
    k = cases("se")
    per = 700
    k.decompress("all", "sp", "-S", per, "--window", REC * 300)
    parts = [read(os.path.join(k.d, "sp.%d_1.fastq" % (i + 1))) for i in range((N + per - 1) // per)]
    assert b"".join(parts) == k.input[0] and [len(cut(p)) for p in parts] == [700, 700, 700, 700, 200]
    r = k.decompress("all", "-", "--window", REC * 500)
    assert r.stdout == k.input[0]


def test_lossless_of_fasta_is_the_three_other_options(cases, tmp_path):
    text = b"".join(b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in cut(cases("se").input[0]))
    src = write(tmp_path / "in_1.fa", text)
    scalce("-f", "-s", "1000", "-c", "no", "--lossless", "-o", tmp_path / "fa", src)
    assert not os.path.exists(tmp_path / "fa_1.scalcep")
    assert all(os.path.exists(tmp_path / ("fa_1.scalce" + e)) for e in "ocx")
    scalce("-d", "-f", "-o", tmp_path / "back", tmp_path / "fa_1.scalcen")
    # (two-line records come back with '@' in front of the name, whatever the input had)
    assert read(tmp_path / "back_1.fastq") == text.replace(b">", b"@")


# ---- --keep-plus alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen", "gz"])
def test_keep_plus_alone_puts_the_entries_into_the_plain_text(name, cases):
    k = cases(name)
    k.decompress("plus", "bp", "--bare-plus")
    k.decompress("plain", "pl")
    k.decompress("plus", "wp")
    bare = k.outputs("bp")
    assert bare == k.outputs("pl")   # --bare-plus: what -d writes without the stream
    ents = [fmt.unpack_plus(F.content(os.path.join(k.d, "plus_%d.scalcep" % (m + 1)))) for m in range(k.files)]
    for m, text in enumerate(k.outputs("wp")):
        assert text == (PR.restore(bare[m], ents, interleaved=True) if name == "il" else PR.restore(bare[m], [ents[m]]))
    # -Q ignores the stream: two-line records have no such line
    if name == "se":
        k.decompress("plus", "q2", "-Q")
        k.decompress("plain", "q0", "-Q")
        assert k.outputs("q2") == k.outputs("q0")
        k.decompress("plus", "nl", "-n", "lib")
        # under -n a repeat expands to the header line as it is written
        lines = k.outputs("nl")[0].split(b"\n")
        reps = [i for i, e in enumerate(ents[0]) if e == b"="]
        assert reps and all(lines[4 * i + 2] == b"+" + lines[4 * i][1:] and lines[4 * i].startswith(b"@lib.") for i in reps[:200])


def test_the_stream_holds_the_inputs_entries_in_archive_order(cases):
    from scalce_amd import host
    for name in ("se", "pe", "il"):
        k = cases(name)
        perm = host.unpack_order(F.content(os.path.join(k.d, "all_1.scalceo")))
        texts = k.mates_text if name == "il" else k.input
        for m, text in enumerate(texts):
            ents = PR.entries(text)[0]
            assert F.content(os.path.join(k.d, "all_%d.scalcep" % (m + 1))) == PR.stream(ents, perm), (name, m)


def test_an_all_bare_input_writes_the_header_alone(cases, tmp_path):
    text = PR.bare(cases("se").input[0])
    src = write(tmp_path / "in_1.fq", text)
    log = scalce("-s", "1000", "-c", "no", "--keep-plus", "-o", tmp_path / "b", src).stderr.decode()
    assert read(tmp_path / "b_1.scalcep") == b"scalce22" + struct.pack("<iiq", 0, 0, N)
    assert "Plus lines: %d records, 0 repeated, 0 literal, longest 0" % N in log
    scalce("-d", "-o", tmp_path / "back", tmp_path / "b_1.scalcen")
    scalce("-d", "--bare-plus", "-o", tmp_path / "back0", tmp_path / "b_1.scalcen")
    assert read(tmp_path / "back_1.fastq") == read(tmp_path / "back0_1.fastq")


# ---- the other files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_other_file_is_the_one_without_the_option(name, cases):
    k = cases(name)
    exts = "rnq" + ("l" if name == "varlen" else "")
    for m in range(k.files):
        for e in exts:
            a, b = (os.path.join(k.d, "%s_%d.scalce%s" % (w, m + 1, e)) for w in ("plain", "plus"))
            assert read(a) == read(b), (m, e)
            assert read(a) == read(os.path.join(k.d, "all_%d.scalce%s" % (m + 1, e))), (m, e)
        assert not os.path.exists(os.path.join(k.d, "plain_%d.scalcep" % (m + 1)))
        data = F.content(os.path.join(k.d, "plus_%d.scalcep" % (m + 1)))
        assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24])[0] == 0 and struct.unpack("<iiq", data[8:24])[2] == k.n
        raw = read(os.path.join(k.d, "plus_%d.scalcep" % (m + 1)))
        assert (raw[:2] == b"\x1f\x8b") == (name == "gz")
    # the log: one line per mate, and none without the option
    got = re.findall(r"Plus lines: (\d+) records, (\d+) repeated, (\d+) literal, longest (\d+)", k.logs["plus"])
    assert len(got) == k.files and "Plus lines:" not in k.logs["plain"]
    for m, (n, rep, lit, longest) in enumerate(got):
        data = F.content(os.path.join(k.d, "plus_%d.scalcep" % (m + 1)))
        ents = fmt.unpack_plus(data)
        assert (int(n), int(rep), int(lit), int(longest)) == (k.n, sum(e == b"=" for e in ents), sum(len(e) > 1 for e in ents),
                                                              struct.unpack("<iiq", data[8:24])[1])


@have_ref
def test_the_reference_writes_the_same_three_files_and_reads_the_archive(cases, tmp_path):
    k = cases("se")
    r = subprocess.run([F.REF_FULL, "compress", F.PBIN, k.ins[0], str(tmp_path / "ref"), "-s", "1000", "-c", "no", "-T", "1", "-t",
                        str(tmp_path / "tmp_ref")], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    for e in "rnq":
        assert read(tmp_path / ("ref_1.scalce" + e)) == read(os.path.join(k.d, "plus_1.scalce" + e)), e
    r = subprocess.run([F.REF_FULL, "decompress", F.PBIN, k.arc("plus"), str(tmp_path / "back"), "-T", "1"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    k.decompress("plus", "bp2", "--bare-plus")
    assert read(tmp_path / "back_1.fastq") == k.outputs("bp2")[0]


# ---- ranges -------------------------------------------------------------------------------------------------------------------
def test_record_ranges_concatenate_to_the_whole(cases, tmp_path):
    k = cases("se")
    k.decompress("plus", "allr")
    whole = k.outputs("allr")[0]
    recs = cut(whole)
    slices = []
    for first, count in ((0, 1), (1, 699), (700, 1), (701, 1500), (2201, N)):
        k.decompress("plus", "rg%d" % first, "--records", "%d:%d" % (first, count), "--window", REC * 300)
        slices.append(k.outputs("rg%d" % first)[0])
        assert slices[-1] == b"".join(recs[first:first + count])
    assert b"".join(slices) == whole
    k.decompress("plus", "rgend", "--records", str(N))
    assert k.outputs("rgend")[0] == b""
    k.decompress("all", "rgao", "--records", "10:5", "--archive-order")
    k.decompress("all", "ao", "--archive-order")
    assert k.outputs("rgao")[0] == b"".join(cut(k.outputs("ao")[0])[10:15])
    # a stream cut short behind the range is not noticed
    data = read(os.path.join(k.d, "plus_1.scalcep"))
    ends = [i for i in range(24, len(data)) if data[i] == 10]
    arc = damaged(k, tmp_path, lambda d: d[:ends[999] + 1])
    scalce("-d", "-o", tmp_path / "front", arc, "--records", "100:900", "--window", REC * 300)
    assert read(tmp_path / "front_1.fastq") == b"".join(recs[100:1000])


# ---- a stale stream -----------------------------------------------------------------------------------------------------------
def test_a_later_run_without_the_option_removes_the_stream(cases, tmp_path):
    k = cases("pe")
    out = tmp_path / "x"
    scalce("-r", *k.common, "--keep-plus", "-o", out, *k.ins)
    assert os.path.exists(tmp_path / "x_1.scalcep") and os.path.exists(tmp_path / "x_2.scalcep")
    scalce("-r", *k.common, "-o", out, *k.ins)
    assert not os.path.exists(tmp_path / "x_1.scalcep") and not os.path.exists(tmp_path / "x_2.scalcep")


# ---- errors -------------------------------------------------------------------------------------------------------------------
def damaged(k, tmp_path, change):
    for ext in "rnqp":
        data = read(os.path.join(k.d, "plus_1.scalce%s" % ext))
        write(tmp_path / ("a_1.scalce%s" % ext), change(data) if ext == "p" else data)
    return tmp_path / "a_1.scalcen"


def fails_with(arc, tmp_path, word, *flags):
    r = scalce("-d", "-o", tmp_path / "out", arc, *flags, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and word in err, err[-800:]


def test_damaged_streams(cases, tmp_path):
    k = cases("se")
    data = read(os.path.join(k.d, "plus_1.scalcep"))
    ends = [i for i in range(24, len(data)) if data[i] == 10]
    window = REC * 200
    inside = next(e for e in ends[1500:] if data[e - 1] != 10 and data[e - 2] != 10) - 1   # inside a literal
    lit = next(i for i in range(len(ends) - 1) if data[ends[i] + 1:ends[i] + 2] == b"'")
    for i, (change, word) in enumerate([
            (lambda d: d[:inside], "truncated plus-line stream"),                                # inside a window, inside an entry
            (lambda d: d[:ends[1500] + 1], "truncated plus-line stream"),                        # between two entries
            (lambda d: d[:20], "truncated plus-line stream"),                                    # inside the header
            (lambda d: d[:24], "truncated plus-line stream"),                                    # the header and nothing else
            (lambda d: b"notscalc" + d[8:], "is not a scalce plus-line stream"),
            (lambda d: d[:8] + struct.pack("<i", 4) + d[12:], "is not a scalce plus-line stream"),
            (lambda d: d[:16] + struct.pack("<q", N - 1) + d[24:], "plus-line stream holds %d entries, the archive %d records" % (N - 1, N)),
            (lambda d: d[:16] + struct.pack("<q", N + 1) + d[24:], "plus-line stream holds %d entries, the archive %d records" % (N + 1, N)),
            (lambda d: d[:12] + struct.pack("<i", 3) + d[16:], "plus-line stream: an entry is longer than its header says"),
            (lambda d: d[:ends[lit] + 1] + b"x" + d[ends[lit] + 2:], "plus-line stream: malformed entry")]):
        sub = tmp_path / ("case%d" % i)
        os.mkdir(sub)
        fails_with(damaged(k, sub, change), sub, word, "--window", window)
    # a stream cut exactly where a window ends: the windows of this size, counted from the log of a whole run
    r = k.decompress("plus", "wn", "--window", window)
    nwin = int(re.search(r"Windows: (\d+)", r.stderr.decode()).group(1))
    assert nwin >= 3
    text = k.outputs("wn")[0]
    recs = cut(text)
    size, first_window = 0, 0
    for rec in recs:   # the first window takes records while their text fits
        if first_window and size + len(rec) > window:
            break
        size += len(rec)
        first_window += 1
    sub = tmp_path / "boundary"
    os.mkdir(sub)
    fails_with(damaged(k, sub, lambda d: d[:ends[first_window - 1] + 1]), sub, "truncated plus-line stream", "--window", window)


def test_refusals(cases, tmp_path):
    k = cases("se")
    for flags, word in ((["--keep-plus", "-f"], "-f"), (["--keep-plus", "-Q"], "-Q"), (["--keep-plus", "--gpus", "2", "-B", "1M"], "--gpus"),
                        (["--keep-plus", "-d"], "--keep-plus"), (["--bare-plus"], "--bare-plus"),
                        (["--lossless", "-p", "10"], "lossy"), (["--lossless", "-n", "lib"], "names"), (["--lossless", "-Q"], "qualities"),
                        (["--lossless", "--gpus", "2", "-B", "1M"], "--gpus"), (["--lossless", "-d"], "--lossless")):
        src = k.arc("plus") if "-d" in flags else k.ins[0]
        r = scalce(*flags, "-c", "no", "-o", tmp_path / "x", src, ok=False)
        err = r.stderr.decode()
        assert r.returncode == 1 and "(ERROR)" in err and word in err, err
        assert os.listdir(tmp_path) == []
    # --lossless with -p 0 and with --variable-length / --max-length is the promise kept
    scalce("--lossless", "-p", "0", "--max-length", L, "-s", "1000", "-c", "no", "-o", tmp_path / "ok", k.ins[0])
    scalce("-d", "-o", tmp_path / "okback", tmp_path / "ok_1.scalcen")
    assert read(tmp_path / "okback_1.fastq") == k.input[0]
