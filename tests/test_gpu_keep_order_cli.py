"""-m gpu: `scalce --keep-order` and the restore of the input order by `scalce -d`, as a program.

Compress: every file of the archive but the .scalceo is byte for byte the one the run without the option writes; the .scalceo
holds a permutation, and record k of the --archive-order output is input record entry[k].  Restore: the expected text is the
--archive-order output (which other tests pin to the reference) cut into records and placed by the entries -- and, where that
run returns its input unchanged, the input files themselves.  Then windows of every size against scalce_order_plan, -S, -o -,
damaged order streams, refusals, and that nothing changes for an archive without the stream.  After every run the -t directory
is empty."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import filecases as F
import varlen_util as V
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
N, L = 3000, 60
REC_MAX = 2 * L + 6 + 255 + 32     # the window loop's bound of a record's text, per mate


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
    """the records of `lines` lines each of a text"""
    ls = text.split(b"\n")
    assert ls[-1] == b"" and (len(ls) - 1) % lines == 0, (len(ls), lines)
    return [b"\n".join(ls[i:i + lines]) + b"\n" for i in range(0, len(ls) - 1, lines)]


def place(text, lines, entries):
    """the records of an --archive-order text at the places the order stream gives them"""
    recs = cut(text, lines)
    assert len(recs) == len(entries)
    out = [None] * len(recs)
    for k, e in enumerate(entries):
        out[e] = recs[k]
    return b"".join(out)


def fastq(n, length, seed, prefix="r.", suffix=""):
    bases, quals = synth.reads_and_quals(n, length, seed=seed, dup_frac=0.2)
    return synth.fastq_bytes_fast(bases, quals, prefix=prefix, suffix=suffix)


def interleaved(a, b):
    return b"".join(x + y for x, y in zip(cut(a, 4), cut(b, 4)))


def fasta_of(text):
    return b"".join(b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in cut(text, 4))


# name -> compress flags, decompress flags, lines per record of the output, mates written, whether -d returns the input itself
CASES = {
    "se": dict(c=[], d=[], lines=4, mates=1, exact=True),
    "pe": dict(c=["-r"], d=["-r"], lines=4, mates=2, exact=True),
    "il": dict(c=["-i"], d=["-i"], lines=8, mates=1, exact=True),
    "Q": dict(c=["-Q"], d=["-Q"], lines=2, mates=1, exact=False),
    "f": dict(c=["-f"], d=["-f"], lines=2, mates=1, exact=False),
    "nlib": dict(c=["-n", "lib"], d=[], lines=4, mates=1, exact=False),
    "A": dict(c=["-A"], d=[], lines=4, mates=1, exact=True),
    "gz": dict(c=["-c", "gz"], d=[], lines=4, mates=1, exact=True),
    "varlen": dict(c=["--variable-length"], d=[], lines=4, mates=1, exact=True),
    "multi": dict(c=[], d=[], lines=4, mates=1, exact=True),
    "B": dict(c=["-B", "1M"], d=[], lines=4, mates=1, exact=True, n=60000, L=100),
}


class Case:
    """a case's input, its archive with and without --keep-order, and the --archive-order text of the former"""

    def __init__(self, name, root):
        self.name, self.c = name, CASES[name]
        self.d = d = str(root.mktemp("ko_" + name))
        self.tdir = os.path.join(d, "spill")
        os.mkdir(self.tdir)
        n, length = self.c.get("n", N), self.c.get("L", L)
        self.n = n
        ins = [os.path.join(d, "in_1.fq")]
        if name == "pe":
            self.input = [fastq(n, length, 31, "p.", "/1"), fastq(n, length, 32, "p.", "/2")]
            write(ins[0], self.input[0])
            write(os.path.join(d, "in_2.fq"), self.input[1])
        elif name == "il":
            self.input = [interleaved(fastq(n, length, 31, "p.", "/1"), fastq(n, length, 32, "p.", "/2"))]
            write(ins[0], self.input[0])
        elif name == "f":
            self.input = [fasta_of(fastq(n, length, 33))]
            write(ins[0], self.input[0])
        elif name == "varlen":
            var, _, _ = V.texts(length, V.lengths_covering(n, length, 34), 35, n_frac=0.0)
            self.input = [var]
            write(ins[0], var)
        elif name == "multi":   # three input files, the second one gzipped: the index runs over all of them in the order given
            text = fastq(n, length, 36)
            recs = cut(text, 4)
            parts = [b"".join(recs[:700]), b"".join(recs[700:1900]), b"".join(recs[1900:])]
            ins = [os.path.join(d, "ina_1.fq"), os.path.join(d, "inb_1.fq.gz"), os.path.join(d, "inc_1.fq")]
            write(ins[0], parts[0])
            write(ins[1], gzip.compress(parts[1], 1))
            write(ins[2], parts[2])
            self.input = [text]
        else:
            self.input = [fastq(n, length, 30 + len(name))]
            write(ins[0], self.input[0])
        common = ["-s", "1000"] + ([] if "-c" in self.c["c"] else ["-c", "no"])
        scalce(*self.c["c"], *common, "-o", os.path.join(d, "plain"), *ins)
        scalce(*self.c["c"], *common, "--keep-order", "-o", os.path.join(d, "kept"), *ins)
        self.arc = os.path.join(d, "kept_1.scalcen")
        self.entries = host.unpack_order(F.content(os.path.join(d, "kept_1.scalceo")))
        scalce("-d", "--archive-order", *self.c["d"], "-o", os.path.join(d, "ao"), self.arc)
        self.ao = [read(os.path.join(d, "ao_%d.fastq" % (m + 1))) for m in range(self.c["mates"])]
        self.want = [place(t, self.c["lines"], self.entries) for t in self.ao]

    def restore(self, out, *flags, ok=True):
        r = scalce("-d", *self.c["d"], "-t", self.tdir, "-o", os.path.join(self.d, out) if out != "-" else "-", self.arc, *flags, ok=ok)
        assert os.listdir(self.tdir) == [], "the spill left a file behind"
        return r

    def got(self, out):
        return [read(os.path.join(self.d, "%s_%d.fastq" % (out, m + 1))) for m in range(self.c["mates"])]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory)
        return made[name]
    return get


def order_line(r):
    m = re.search(r"Order: (\d+) records restored through (\d+) stripes of up to (\d+) records; (\d+) bytes spilled in (\S+)", r.stderr.decode())
    assert m, r.stderr[-800:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)


# ---- compress -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen", "gz"])
def test_archive_is_the_one_without_the_option_plus_the_order_stream(name, cases):
    k = cases(name)
    exts = "rnq" + ("l" if name == "varlen" else "")
    for m in range(2 if name in ("pe", "il") else 1):
        for e in exts:
            a, b = (os.path.join(k.d, "%s_%d.scalce%s" % (p, m + 1, e)) for p in ("plain", "kept"))
            assert F.content(a) == F.content(b) and read(a)[:2] == read(b)[:2], "%s: .scalce%s of mate %d" % (name, e, m + 1)
    assert not os.path.exists(os.path.join(k.d, "plain_1.scalceo")) and not os.path.exists(os.path.join(k.d, "kept_2.scalceo"))
    raw = read(os.path.join(k.d, "kept_1.scalceo"))
    assert (raw[:2] == b"\x1f\x8b") == (name == "gz")
    data = F.content(os.path.join(k.d, "kept_1.scalceo"))
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (4, 0, k.n) and len(data) == 24 + 4 * k.n
    assert (np.sort(k.entries) == np.arange(k.n)).all(), "the entries are a permutation of the records (pairs)"
    assert (k.entries != np.arange(k.n)).any(), "the archive is in bucket order, not in the input's"
    # record k of the archive is input record entry[k]: by name (mate 1's; the input's records are four lines each)
    names_in = [r.split(b"\n")[0] for r in cut(k.input[0], 4)][:: 2 if name == "il" else 1]
    names_ao = [r.split(b"\n")[0] for r in cut(k.ao[0], k.c["lines"])]
    assert names_ao == [names_in[e] for e in k.entries]


# ---- restore ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restore_gives_the_input_order(name, cases):
    k = cases(name)
    r = k.restore("back")
    assert k.got("back") == k.want
    if k.c["exact"]:
        assert k.got("back") == k.input, "a lossless run with names returns the input files themselves"
    n, S, R, spilled, where = order_line(r)
    assert n == k.n and S == 1 and where == k.tdir
    assert spilled == (sum(len(t) for t in k.ao) + 8 * k.n * k.c["mates"])


def test_several_spill_chunks_were_made(cases):
    k = cases("B")
    r = scalce("-B", "1M", "-s", "1000", "-c", "no", "--keep-order", "-o", os.path.join(k.d, "again"), os.path.join(k.d, "in_1.fq"))
    line = next(ln for ln in r.stderr.decode().splitlines() if "Spill chunks" in ln)
    assert int(line.split("Spill chunks:")[1].split(",")[0]) >= 2, line
    assert read(os.path.join(k.d, "again_1.scalceo")) == read(os.path.join(k.d, "kept_1.scalceo"))


def test_made_up_names_keep_the_archives_index(cases):
    k = cases("nlib")
    names = [r.split(b"\n")[0] for r in cut(k.want[0], 4)]
    assert sorted(names) == sorted(b"@lib.%d" % i for i in range(N)) and names != [b"@lib.%d" % i for i in range(N)]
    assert [int(x.split(b".")[1]) for x in names] == list(np.argsort(k.entries))   # input record e carries the archive index k


@pytest.mark.parametrize("name", ["se", "pe"])
@pytest.mark.parametrize("window", [1, 10 * (2 * L + 6 + 8), "third", None], ids=["one_record", "ten_records", "a_third", "default"])
def test_windows_of_every_size_give_the_same_bytes(window, name, cases):
    k = cases(name)
    if window == "third":
        window = len(k.ao[0]) // 3 + 200
    out = "w_%s" % window
    r = k.restore(out, *([] if window is None else ["--window", window]))
    assert k.got(out) == k.want
    n, S, R, _, _ = order_line(r)
    assert (R, S) == host.order_plan(N, window or (1 << 30), REC_MAX) and n == N
    if window == 1:
        assert (R, S) == (1, N)
    if window is None:
        assert S == 1


def test_split_parts_concatenate_to_the_whole(cases):
    k = cases("se")
    r = k.restore("sp", "-S", 700, "--window", REC_MAX * 300)      # stripes of 300 records: part boundaries lie inside stripes
    assert order_line(r)[1:3] == (10, 300)
    parts = [read(os.path.join(k.d, "sp.%d_1.fastq" % (i + 1))) for i in range(5)]
    assert [len(cut(p, 4)) for p in parts] == [700, 700, 700, 700, 200]
    assert b"".join(parts) == k.want[0]
    assert not os.path.exists(os.path.join(k.d, "sp.6_1.fastq"))


def test_split_counts_pairs_under_interleave(cases):
    k = cases("il")
    k.restore("spi", "-S", 1100, "--window", 2 * REC_MAX * 250)
    parts = [read(os.path.join(k.d, "spi.%d_1.fastq" % (i + 1))) for i in range(3)]
    assert [len(cut(p, 8)) for p in parts] == [1100, 1100, 800] and b"".join(parts) == k.want[0]


def test_stdout(cases):
    k = cases("se")
    r = k.restore("-", "--window", REC_MAX * 1000)
    assert r.stdout == k.want[0]


def test_spill_goes_next_to_the_output_without_t(cases, tmp_path):
    k = cases("se")
    r = scalce("-d", "-o", tmp_path / "o", k.arc, "--window", REC_MAX * 500)
    assert read(tmp_path / "o_1.fastq") == k.want[0]
    assert order_line(r)[4] == str(tmp_path) and sorted(os.listdir(tmp_path)) == ["o_1.fastq"]


# ---- errors and refusals ------------------------------------------------------------------------------------------------------
def damaged(k, tmp_path, change):
    for ext in "rnqo":
        data = read(os.path.join(k.d, "kept_1.scalce%s" % ext))
        write(tmp_path / ("a_1.scalce%s" % ext), change(data) if ext == "o" else data)
    return tmp_path / "a_1.scalcen"


def fails_with(k, arc, tmp_path, message, *flags):
    r = scalce("-d", "-t", k.tdir, "-o", tmp_path / "o", arc, *flags, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and message in err, err[-600:]
    assert os.listdir(k.tdir) == []


@pytest.mark.parametrize("window", [1, None], ids=["one_record", "default"])
@pytest.mark.parametrize("keep", [7, 23, 24 + 4 * 1500 + 2, 24 + 4 * N - 1], ids=["in_magic", "header_but_a_byte", "inside_an_entry", "last_byte"])
def test_order_stream_cut_short(keep, window, cases, tmp_path):
    k = cases("se")
    fails_with(k, damaged(k, tmp_path, lambda data: data[:keep]), tmp_path, "truncated order stream", *([] if window is None else ["--window", window]))


def test_order_stream_without_entries_or_bytes(cases, tmp_path):
    k = cases("se")
    fails_with(k, damaged(k, tmp_path, lambda data: data[:24]), tmp_path, "truncated order stream", "--window", REC_MAX * 100)
    fails_with(k, damaged(k, tmp_path, lambda data: b""), tmp_path, "truncated order stream", "--window", REC_MAX * 100)


def test_order_stream_of_another_kind(cases, tmp_path):
    k = cases("se")
    w = ["--window", REC_MAX * 100]
    fails_with(k, damaged(k, tmp_path, lambda data: b"notscalc" + data[8:]), tmp_path, "is not a scalce order stream", *w)
    fails_with(k, damaged(k, tmp_path, lambda data: data[:8] + struct.pack("<i", 8) + data[12:]), tmp_path, "is not a scalce order stream", *w)


# what is wrong with the entries, at windows that find it in the window loop (an entry beyond the records), in the stripe loop
# by its count (one record per stripe) and in the stripe loop on the device (one stripe: two records claim one place)
@pytest.mark.parametrize("window", [1, REC_MAX * 100, None], ids=["one_record", "hundred_records", "default"])
@pytest.mark.parametrize("at,value", [(10, "entry 2000"), (1234, N)], ids=["duplicate", "beyond_the_records"])
def test_entries_that_are_no_permutation(at, value, window, cases, tmp_path):
    k = cases("se")
    x = k.entries.astype("<u4")
    x[at] = x[2000] if value == "entry 2000" else value
    fails_with(k, damaged(k, tmp_path, lambda data: data[:24] + x.tobytes()), tmp_path, "order stream is not a permutation of the records",
               *([] if window is None else ["--window", window]))


@pytest.mark.parametrize("n", [N - 1, N + 1])
def test_header_count_off_by_one(n, cases, tmp_path):
    k = cases("se")
    arc = damaged(k, tmp_path, lambda data: data[:16] + struct.pack("<q", n) + data[24:])
    fails_with(k, arc, tmp_path, "order stream holds %d entries, the archive %d records" % (n, N), "--window", REC_MAX * 100)


@pytest.mark.parametrize("n", [N - 1, N + 1])
def test_header_count_off_by_one_where_the_archive_does_not_say_its_count(n, cases, tmp_path):
    """-A: no symbol count; the difference shows where the streams end"""
    a = cases("A")
    for ext in "rnq":
        write(tmp_path / ("b_1.scalce%s" % ext), read(os.path.join(a.d, "kept_1.scalce%s" % ext)))
    data = read(os.path.join(a.d, "kept_1.scalceo"))
    # (one entry more, or the stream of the first N - 1 input records: the count alone is wrong, every entry names a record)
    body = data[24:] + b"\0\0\0\0" if n > N else a.entries[a.entries != N - 1].astype("<u4").tobytes()
    write(tmp_path / "b_1.scalceo", data[:16] + struct.pack("<q", n) + body)
    want = "order stream holds %d entries, the archive %d records" % (n, N) if n > N else "order stream holds %d entries, the archive more" % n
    fails_with(a, tmp_path / "b_1.scalcen", tmp_path, want, "--window", REC_MAX * 700)


def test_records_needs_archive_order(cases, tmp_path):
    k = cases("se")
    r = scalce("-d", "--records", "10:5", "-o", tmp_path / "x", k.arc, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and "--archive-order" in err and "--records" in err
    scalce("-d", "--records", "10:5", "--archive-order", "-o", tmp_path / "y", k.arc)
    scalce("-d", "--records", "10:5", "-o", tmp_path / "z", os.path.join(k.d, "plain_1.scalcen"))
    assert read(tmp_path / "y_1.fastq") == read(tmp_path / "z_1.fastq") == b"".join(cut(k.ao[0], 4)[10:15])


def test_refusals_leave_no_archive(cases, tmp_path):
    k = cases("se")
    src = os.path.join(k.d, "in_1.fq")
    for flags, word in ((["--keep-order", "--gpus", "2", "-c", "no", "-B", "1M"], "--gpus"), (["--keep-order", "-d"], "--keep-order")):
        r = scalce(*flags, "-o", tmp_path / "x", src if "-d" not in flags else k.arc, ok=False)
        err = r.stderr.decode()
        assert r.returncode == 1 and "(ERROR)" in err and word in err and "--keep-order" in err
        assert os.listdir(tmp_path) == []
    r = scalce("--archive-order", "-c", "no", "-o", tmp_path / "x", src, ok=False)
    assert r.returncode == 1 and "--archive-order" in r.stderr.decode() and os.listdir(tmp_path) == []


def test_temp_directory_that_cannot_be_made(cases, tmp_path):
    k = cases("se")
    write(tmp_path / "file", b"x")
    r = scalce("-d", "-t", tmp_path / "file" / "sub", "-o", tmp_path / "o", k.arc, ok=False)
    assert r.returncode == 1 and "(ERROR)" in r.stderr.decode() and str(tmp_path / "file" / "sub") in r.stderr.decode()
    r = scalce("-d", "-t", tmp_path / "file", "-o", tmp_path / "o", k.arc, ok=False)     # there, but no directory: the spill cannot be made
    assert r.returncode == 1 and "(ERROR)" in r.stderr.decode() and "spill" in r.stderr.decode() and str(tmp_path / "file") in r.stderr.decode()
    made = tmp_path / "made_on_demand"
    scalce("-d", "-t", made, "-o", tmp_path / "ok", k.arc)
    assert os.listdir(made) == [] and read(tmp_path / "ok_1.fastq") == k.want[0]


# ---- unchanged ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe"])
def test_an_archive_without_the_stream_decodes_as_before(name, cases, tmp_path):
    k = cases(name)
    plain = os.path.join(k.d, "plain_1.scalcen")
    scalce("-d", *k.c["d"], "-o", tmp_path / "a", plain)
    r = scalce("-d", *k.c["d"], "--archive-order", "-o", tmp_path / "b", plain)
    for m in range(k.c["mates"]):
        assert read(tmp_path / ("a_%d.fastq" % (m + 1))) == read(tmp_path / ("b_%d.fastq" % (m + 1))) == k.ao[m]
    assert "Order:" not in r.stderr.decode()
    assert not any(f.endswith(".scalceo") for f in os.listdir(tmp_path)) and not os.path.exists(os.path.join(k.d, "plain_1.scalceo"))


# ---- the library call through the Python host ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il"])
def test_stream_decompress_restore_through_the_python_host(name, cases, tmp_path):
    """scalce_stream_decompress_restore on the files the CLI read: stripes arrive in input order, first_record rising by the
    stripe's records, and the order stream is read from its start once per mate pass"""
    k = cases(name)
    mates = 2 if name in ("pe", "il") else 1

    def reader(path):
        f = open(path, "rb")
        return lambda cap: f.read(cap)
    readers = [[reader(os.path.join(k.d, "kept_%d.scalce%s" % (m + 1, e))) for e in "rnq"] for m in range(mates)]
    order = [reader(os.path.join(k.d, "kept_1.scalceo")) for _ in range(1 if name == "il" else mates)]
    got = {}
    ctx = host.Context(0, patterns_bin=read(F.PBIN))
    window = (mates if name == "il" else 1) * REC_MAX * 400
    st = host.stream_decompress_restore(ctx, readers, order, lambda mate, first, n, text, offs: got.setdefault(mate, []).append((first, n, text)),
                                        str(tmp_path), mates=mates, interleave=name == "il", window_text_bytes=window)
    ctx.close()
    assert os.listdir(tmp_path) == []
    assert (st.restore.stripe_records, st.restore.stripes) == host.order_plan(N, window, (mates if name == "il" else 1) * REC_MAX) == (400, 8)
    assert st.restore.records == N and st.restore.spilled_bytes == sum(len(t) for t in k.ao) + 8 * N * len(k.ao)
    for m in range(len(k.want)):
        assert [(f, n) for f, n, _ in got[m]] == [(s * 400, min(400, N - s * 400)) for s in range(8)]
        assert b"".join(t for _, _, t in got[m]) == k.want[m]
