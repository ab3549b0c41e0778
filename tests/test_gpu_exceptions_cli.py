"""-m gpu: `scalce --keep-bases` and the bases put back by `scalce -d`, as a program.

Round trip: --keep-order --keep-comments --keep-bases, then -d, gives the input file byte for byte under -p 0, for inputs with
lower-case and IUPAC letters, N under any quality and the lowest quality under any base.  Every other file of the archive is
the one the run without the option writes, the .scalcex holds exception_ref's entries in the archive's order, and the
reference's own decompress() reads the archive.  Then windows, ranges, -S, -o -, -Q, -n, a lossy map, a stale stream, damaged
streams and refusals."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import exception_ref as ER
import filecases as F
from scalce_amd import format as fmt
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
have_ref = pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")
N, L = 20000, 100
REC = 2 * L + 6 + 20   # about a record with its name and comment


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


def letters(n, length, seed):
    """filecases' `letters` case -- soft-masked stretches, whole reads in lower case, IUPAC letters -- plus N with '#' and with
    '!', and '!' under arbitrary bases"""
    bases, quals = synth.reads_and_quals(n, length, seed=seed, dup_frac=0.2)
    bases, quals = bases.copy(), quals.copy()
    rng = np.random.default_rng(seed + 1000)
    low = rng.random(bases.shape) < 0.05
    low[rng.integers(0, n, 40), :] = True
    bases = np.where(low, bases | 0x20, bases)
    amb = np.frombuffer(b"RYKMSWBDHVUXryksw", dtype=np.uint8)
    hit = rng.random(bases.shape) < 0.01
    bases = np.where(hit, amb[rng.integers(0, len(amb), bases.shape)], bases)
    isn = rng.random(bases.shape) < 0.02
    bases[isn] = ord("N")
    quals[isn] = np.where(rng.random(int(isn.sum())) < 0.5, ord("#"), ord("!"))
    quals[rng.random(bases.shape) < 0.01] = ord("!")
    return bases, quals


def fastq(bases, quals, mate=1, slash=False, lens=None, fasta=False):
    out = []
    for r in range(len(bases)):
        k = bases.shape[1] if lens is None else int(lens[r])
        h = b"@r.%d" % r + ((b"/%d" % mate) if slash else b"") + (b" %d:N:0:ACGT" % mate if r % 3 else b"")
        b = bases[r, :k].tobytes()
        out.append(h + b"\n" + b + b"\n" if fasta else h + b"\n" + b + b"\n+\n" + quals[r, :k].tobytes() + b"\n")
    return b"".join(out)


def interleaved(a, b):
    return b"".join(x + y for x, y in zip(cut(a, 4), cut(b, 4)))


CASES = {
    "se": dict(c=[], d=[], lines=4, mates=1),
    "pe": dict(c=["-r"], d=["-r"], lines=4, mates=2),
    "il": dict(c=["-i"], d=["-i"], lines=8, mates=1),
    "f": dict(c=["-f"], d=["-f"], lines=2, mates=1),
    "varlen": dict(c=["--variable-length"], d=[], lines=4, mates=1),
    "gz": dict(c=["-c", "gz"], d=[], lines=4, mates=1),
    "p30": dict(c=["-p", "30"], d=[], lines=4, mates=1),
}
ALL = ["--keep-order", "--keep-comments", "--keep-bases"]


class Case:
    """a case's input and its archives: plain, --keep-bases, and all three --keep options"""

    def __init__(self, name, root):
        self.name, self.c = name, CASES[name]
        self.d = d = str(root.mktemp("kb_" + name))
        ins = [os.path.join(d, "in_1.fq")]
        self.lens = None
        if name in ("pe", "il"):
            self.arrays = [letters(N, L, 31), letters(N, L, 32)]
            self.mates_text = [fastq(*self.arrays[0], 1, True), fastq(*self.arrays[1], 2, True)]
            if name == "pe":
                self.input = self.mates_text
                write(os.path.join(d, "in_2.fq"), self.input[1])
            else:
                self.input = [interleaved(*self.mates_text)]
        elif name == "f":
            self.arrays = [letters(N, L, 33)]
            self.input = [fastq(*self.arrays[0], fasta=True)]
        elif name == "varlen":
            self.lens = np.random.default_rng(34).integers(0, L + 1, size=N)
            self.lens[:L + 1] = np.arange(L + 1)
            self.arrays = [letters(N, L, 35)]
            self.input = [fastq(*self.arrays[0], lens=self.lens)]
        else:
            self.arrays = [letters(N, L, 30 + len(name))]
            self.input = [fastq(*self.arrays[0])]
        write(ins[0], self.input[0])
        self.ins = ins
        self.common = ["-s", "1000"] + ([] if "-c" in self.c["c"] else ["-c", "no"])
        self.logs = {}
        for out, flags in (("plain", []), ("kb", ["--keep-bases"]), ("all", ALL)):
            self.logs[out] = scalce(*self.c["c"], *self.common, *flags, "-o", os.path.join(d, out), *ins).stderr.decode()
        self.files = 2 if name in ("pe", "il") else 1    # mates the archive holds

    def arc(self, which):
        return os.path.join(self.d, which + "_1.scalcen")

    def decompress(self, which, out, *flags, ok=True):
        return scalce("-d", *self.c["d"], "-o", os.path.join(self.d, out) if out != "-" else "-", self.arc(which), *flags, ok=ok)

    def outputs(self, out):
        return [read(os.path.join(self.d, "%s_%d.fastq" % (out, m + 1))) for m in range(self.c["mates"])]

    def stream(self, which, m=0):
        return F.content(os.path.join(self.d, "%s_%d.scalcex" % (which, m + 1)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory)
        return made[name]
    return get


# ---- round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il", "gz", "varlen", "f"])
def test_the_three_keep_options_return_the_input(name, cases):
    k = cases(name)
    k.decompress("all", "rt")
    assert k.outputs("rt") == k.input
    k.decompress("all", "sb", "--stored-bases")
    assert k.outputs("sb") != k.input


def test_stored_bases_is_what_the_archive_without_the_option_gives(cases):
    k = cases("se")
    k.decompress("kb", "sb", "--stored-bases")
    k.decompress("plain", "pl")
    assert k.outputs("sb") == k.outputs("pl")
    # ... and it is the rule's plain text: the entries put into it give what -d writes with them
    k.decompress("kb", "wb")
    L_, n, ents = host.unpack_exceptions(k.stream("kb"))
    assert (L_, n) == (L, N)
    assert b"".join(ER.apply_text(cut(k.outputs("pl")[0], 4), ents, L, True)) == k.outputs("wb")[0]


# ---- the other files ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_other_file_is_the_one_without_the_option(name, cases):
    k = cases(name)
    exts = "rnq" + ("l" if name == "varlen" else "")
    got = re.findall(r"Bases: (\d+) exceptions in (\d+) of (\d+) records", k.logs["kb"])
    assert len(got) == k.files and "Bases:" not in k.logs["plain"]
    for m in range(k.files):
        for e in exts:
            a, b = (os.path.join(k.d, "%s_%d.scalce%s" % (w, m + 1, e)) for w in ("plain", "kb"))
            assert read(a) == read(b), (m, e)
            assert read(a) == read(os.path.join(k.d, "all_%d.scalce%s" % (m + 1, e))), (m, e)
        assert not os.path.exists(os.path.join(k.d, "plain_%d.scalcex" % (m + 1)))
        data = k.stream("kb", m)
        width, rl, n, x = struct.unpack("<iiqq", data[8:32])
        assert data[:8] == b"scalce22" and (width, rl, n) == (8, L, N) and len(data) == 32 + 8 * x
        assert (read(os.path.join(k.d, "kb_%d.scalcex" % (m + 1)))[:2] == b"\x1f\x8b") == (name == "gz")
        assert data == k.stream("all", m)
        assert tuple(map(int, got[m])) == (x, len(np.unique(np.frombuffer(data, dtype="<u8", offset=32) >> np.uint64(28))), N)


@pytest.mark.parametrize("name", ["se", "pe", "il", "f", "varlen", "p30"])
def test_the_stream_holds_the_inputs_exceptions_in_archive_order(name, cases):
    k = cases(name)
    perm = host.unpack_order(F.content(os.path.join(k.d, "all_1.scalceo")))
    texts = k.mates_text if name in ("pe", "il") else k.input
    for m, (bases, quals) in enumerate(k.arrays):
        off, vals = 33, ER.IDENTITY
        if name == "p30":
            off, vals, _ = fmt.sample_qmap(texts[m], sample=1000, lossy=30)
        want = ER.entries(bases, None if name == "f" else quals, off, vals, perm=perm, lens=k.lens)
        assert k.stream("all", m) == ER.pack(want, L, N), (name, m)
        assert len(want) > N


@have_ref
def test_the_reference_reads_the_archive(cases, tmp_path):
    k = cases("se")
    r = subprocess.run([F.REF_FULL, "decompress", F.PBIN, k.arc("kb"), str(tmp_path / "back"), "-T", "1"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    k.decompress("kb", "sb2", "--stored-bases")
    assert read(tmp_path / "back_1.fastq") == k.outputs("sb2")[0]


# ---- a lossy map --------------------------------------------------------------------------------------------------------------
def test_under_a_lossy_map_the_letters_are_the_inputs_and_the_qualities_the_maps(cases):
    k = cases("p30")
    k.decompress("all", "rt")
    bases, quals = k.arrays[0]
    got_b, got_q = ER.parse(k.outputs("rt")[0])
    off, vals, _ = fmt.sample_qmap(k.input[0], sample=1000, lossy=30)
    assert (np.asarray(vals) != np.arange(128)).any()
    assert (got_b == bases).all() and (got_q == ER.mapped(quals, vals)).all()
    assert [r.split(b"\n")[0] for r in cut(k.outputs("rt")[0], 4)] == [r.split(b"\n")[0] for r in cut(k.input[0], 4)]
    k.decompress("all", "sb", "--stored-bases")
    plain_b, plain_q = ER.plain(bases, quals, off, vals)
    sb_b, sb_q = ER.parse(k.outputs("sb")[0])
    assert (sb_b == plain_b).all() and (sb_q == plain_q).all() and (sb_b != bases).sum() > N


# ---- windows and ranges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen"])
@pytest.mark.parametrize("window", [1, 65536], ids=["one_record", "64K"])
def test_windows_of_every_size_give_the_same_text(window, name, cases):
    k = cases(name)
    if window == 1:     # a window per record: the archive's first 300 records, against the input's own records
        k.decompress("all", "w1", "--archive-order", "--records", "0:300", "--window", 1)
        perm = host.unpack_order(F.content(os.path.join(k.d, "all_1.scalceo")))[:300]
        for m, text in enumerate(k.input):
            recs = cut(text, k.c["lines"])
            assert k.outputs("w1")[m] == b"".join(recs[int(p)] for p in perm), (name, m)
        return
    k.decompress("all", "wo%d" % window, "--window", window)
    assert k.outputs("wo%d" % window) == k.input


# ---- compositions on the way in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["A", "T", "B", "two_files", "gz_input", "pieces"])
def test_compress_side_compositions_return_the_input(how, cases, tmp_path):
    """-A, -T, -B (several spill chunks), several input files, gzip input, and an input streamed in several pieces (the store
    grows piece by piece): the round trip gives the input, the stream is the plain run's"""
    k = cases("se")
    ins, flags, env = k.ins, [], dict(os.environ)
    if how == "A":
        flags = ["-A"]
    elif how == "T":
        flags = ["-T", "2"]
    elif how == "B":
        flags = ["-B", "1M"]
    elif how == "two_files":
        recs = cut(k.input[0], 4)
        ins = [write(tmp_path / "ina_1.fq", b"".join(recs[:7001])), write(tmp_path / "inb_1.fq", b"".join(recs[7001:]))]
    elif how == "gz_input":
        ins = [write(tmp_path / "in_1.fq.gz", gzip.compress(k.input[0], 1))]
    else:
        env["SCALCE_PIECE_BYTES"] = str(1 << 20)       # about five pieces of the 4.8 MB input
    out = tmp_path / "c"
    r = subprocess.run([F.SCALCE, *flags, *k.common, *ALL, "-o", str(out), *ins, "--patterns-bin", F.PBIN], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-1500:]
    if how == "pieces":
        assert int(re.search(r"pieces streamed: (\d+)", r.stderr.decode()).group(1)) >= 4
    if how in ("T", "two_files", "gz_input", "pieces"):   # (the same archive order: the same stream, byte for byte)
        assert F.content(str(out) + "_1.scalcex") == k.stream("all")
    else:
        host.unpack_exceptions(F.content(str(out) + "_1.scalcex"))
    scalce("-d", "-o", tmp_path / "back", str(out) + "_1.scalcen")
    assert read(tmp_path / "back_1.fastq") == k.input[0]


def test_record_ranges_concatenate_to_the_whole(cases):
    k = cases("se")
    k.decompress("kb", "whole")
    whole = k.outputs("whole")[0]
    recs = cut(whole, 4)
    slices = []
    for first, count in ((0, 1), (1, 6999), (7000, 1), (7001, 9000), (16001, N)):
        k.decompress("kb", "rg%d" % first, "--records", "%d:%d" % (first, count), "--window", REC * 3000)
        slices.append(k.outputs("rg%d" % first)[0])
        assert slices[-1] == b"".join(recs[first:first + count])
    assert b"".join(slices) == whole
    k.decompress("kb", "rgend", "--records", str(N))
    assert k.outputs("rgend")[0] == b""
    k.decompress("all", "rgao", "--records", "10:5", "--archive-order", "--no-comments")
    assert k.outputs("rgao")[0] == b"".join(recs[10:15])


def test_split_parts_and_stdout(cases):
    k = cases("se")
    per = 7000
    k.decompress("all", "sp", "-S", per, "--window", REC * 3000)
    parts = [read(os.path.join(k.d, "sp.%d_1.fastq" % (i + 1))) for i in range((N + per - 1) // per)]
    assert b"".join(parts) == k.input[0] and [len(cut(p, 4)) for p in parts] == [7000, 7000, 6000]
    r = k.decompress("all", "-", "--window", REC * 5000)
    assert r.stdout == k.input[0]


# ---- without qualities or names on the way out --------------------------------------------------------------------------------
def test_dropping_the_qualities_on_the_way_out_applies_the_letters(cases):
    """-d -Q on an archive made with qualities: the letters go back; an N that rests on the undecoded qualities -- one whose
    quality is the offset, no exception -- still comes back as A"""
    k = cases("se")
    k.decompress("all", "nq", "-Q")
    bases, quals = k.arrays[0]
    got, _ = ER.parse(k.outputs("nq")[0], 2)
    rests = (bases == ord("N")) & (quals == ord("!"))
    assert rests.sum() > 100 and (got[rests] == ord("A")).all() and (got[~rests] == bases[~rests]).all()


def test_made_up_names(cases):
    for name in ("se", "il"):
        k = cases(name)
        k.decompress("all", "lib", "-n", "lib", "--archive-order")
        k.decompress("all", "libsb", "-n", "lib", "--archive-order", "--stored-bases")
        lines = k.c["lines"]
        ents = [host.unpack_exceptions(k.stream("all", m))[2] for m in range(k.files)]
        recs = cut(k.outputs("libsb")[0], 4)
        want = ER.apply_text(recs, ents[0], L, True, stride=lines // 4, which=0)
        if name == "il":
            want = ER.apply_text(want, ents[1], L, True, stride=2, which=1)
        assert k.outputs("lib")[0] == b"".join(want)


# ---- a stale stream -----------------------------------------------------------------------------------------------------------
def test_a_later_run_without_the_option_removes_the_stream(cases, tmp_path):
    k = cases("pe")
    out = tmp_path / "x"
    scalce("-r", *k.common, "--keep-bases", "-o", out, *k.ins)
    assert os.path.exists(tmp_path / "x_1.scalcex") and os.path.exists(tmp_path / "x_2.scalcex")
    scalce("-r", *k.common, "-o", out, *k.ins)
    assert not os.path.exists(tmp_path / "x_1.scalcex") and not os.path.exists(tmp_path / "x_2.scalcex")


# ---- errors -------------------------------------------------------------------------------------------------------------------
def damaged(k, tmp_path, change):
    for ext in "rnqx":
        data = read(os.path.join(k.d, "kb_1.scalce%s" % ext))
        write(tmp_path / ("a_1.scalce%s" % ext), change(data) if ext == "x" else data)
    return tmp_path / "a_1.scalcen"


def fails_with(arc, tmp_path, word, *flags):
    r = scalce("-d", "-o", tmp_path / "out", arc, *flags, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and word in err, err[-800:]


def test_damaged_streams(cases, tmp_path):
    k = cases("se")
    e = np.frombuffer(k.stream("kb"), dtype="<u8", offset=32)
    mid = len(e) // 2
    far =struct.pack("<Q", (N << 28) | ord("n"))                            # the last entry: a record the archive does not hold
    for i, (change, word) in enumerate([
            (lambda d: d[:32 + 8 * mid + 3], "truncated exception stream"),                 # inside an entry
            (lambda d: d[:32 + 8 * mid], "truncated exception stream"),                     # between two entries
            (lambda d: d[:20], "truncated exception stream"),
            (lambda d: b"notscalc" + d[8:], "is not a scalce exception stream"),
            (lambda d: d[:8] + struct.pack("<i", 4) + d[12:], "is not a scalce exception stream"),
            (lambda d: d[:16] + struct.pack("<q", N - 1) + d[24:], "exception stream holds %d records, the archive %d" % (N - 1, N)),
            (lambda d: d[:16] + struct.pack("<q", N + 1) + d[24:], "exception stream holds %d records, the archive %d" % (N + 1, N)),
            (lambda d: d[:12] + struct.pack("<i", L + 1) + d[16:], "exception stream is for reads of %d bases, the archive's have %d" % (L + 1, L)),
            (lambda d: d[:32 + 8 * mid] + d[32 + 8 * mid + 8:32 + 8 * mid + 16] + d[32 + 8 * mid:32 + 8 * mid + 8] + d[32 + 8 * mid + 16:],
             "exception stream: entries are not in ascending order"),
            (lambda d: d[:-8] + far, "exception stream: an entry lies outside its record")]):
        sub = tmp_path / ("case%d" % i)
        os.mkdir(sub)
        fails_with(damaged(k, sub, change), sub, word, "--window", REC * 2000)
    # ... and --stored-bases does not look at the stream
    sub = tmp_path / "ignored"
    os.mkdir(sub)
    scalce("-d", "-o", sub / "out", damaged(k, sub, lambda d: d[:20]), "--stored-bases")


def test_refusals(cases, tmp_path):
    k = cases("se")
    for flags, word in ((["--keep-bases", "--gpus", "2", "-B", "1M"], "--gpus"), (["--keep-bases", "-d"], "--keep-bases"),
                        (["--stored-bases"], "--stored-bases")):
        src = k.arc("kb") if "-d" in flags else k.ins[0]
        r = scalce(*flags, "-c", "no", "-o", tmp_path / "x", src, ok=False)
        err = r.stderr.decode()
        assert r.returncode == 1 and "(ERROR)" in err and word in err, err
        assert os.listdir(tmp_path) == []
