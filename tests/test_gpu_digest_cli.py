"""-m gpu: `scalce --lossless --digest`, the check `scalce -d` makes by itself, and `-d --test`, as a program.

The .scalced holds len(input) and zlib.crc32(input) of every text the run read; every other file is the one --lossless alone
writes; -d logs the match and returns the input.  Then many windows and stripes, -S parts, the shapes of input (-r, -i, -f,
--variable-length, two files, -c gz, gzip input with one member and with several), tampered archives, --test, the options under
which the text is not the input's, refusals, and a stale stream."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import filecases as F
from scalce_amd import format as fmt
from scalce_amd import synth

pytestmark = pytest.mark.gpu
N, L = 2000, 60
REC = 2 * (2 * L + 6 + 60)


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
    assert ls[-1] == b"" and (len(ls) - 1) % lines == 0
    return [b"\n".join(ls[i:i + lines]) + b"\n" for i in range(0, len(ls) - 1, lines)]


def fastq(n, length, seed, mate=1, lens=None, fasta=False):
    """records with comments, '+' lines of three kinds, lower-case and IUPAC letters: what only --lossless brings back"""
    bases, quals = synth.reads_and_quals(n, length, seed=seed, dup_frac=0.2, n_frac=0.01)
    rng = np.random.default_rng(seed + 1000)
    odd = np.frombuffer(b"acgtnRYKMSWN", dtype=np.uint8)
    where = rng.random(bases.shape) < 0.02
    bases = np.where(where, odd[rng.integers(0, len(odd), size=bases.shape)], bases).astype(np.uint8)
    out = []
    for r in range(n):
        k = length if lens is None else int(lens[r])
        h = b"SRR1.%d/%d" % (r, mate) + (b"" if r % 5 == 4 else b" lane=%d length=%d" % (r % 8, k))
        if fasta:
            out.append(b"@" + h + b"\n" + bases[r, :k].tobytes() + b"\n")
        else:
            third = (b"+" + h, b"+", b"+other")[r % 3]
            out.append(b"@" + h + b"\n" + bases[r, :k].tobytes() + b"\n" + third + b"\n" + quals[r, :k].tobytes() + b"\n")
    return b"".join(out)


# name -> compress flags, decompress flags
CASES = {
    "se": dict(c=[], d=[]),
    "pe": dict(c=["-r"], d=["-r"]),
    "il": dict(c=["-i"], d=["-i"]),
    "fa": dict(c=["-f"], d=["-f"]),
    "varlen": dict(c=["--variable-length"], d=[]),
    "two": dict(c=[], d=[]),
    "gz": dict(c=["-c", "gz"], d=[]),
    "gzin": dict(c=[], d=[]),
    "gzmulti": dict(c=[], d=[]),
}
KIND = {"pe": 1, "il": 2, "fa": 4}


class Case:
    """a case's input texts (one per mate stream) and its two archives: --lossless ("all") and --lossless --digest ("dig")"""

    def __init__(self, name, root):
        self.name, self.c = name, CASES[name]
        self.d = d = str(root.mktemp("dg_" + name))
        ins = [os.path.join(d, "in_1.fq")]
        if name == "pe":
            self.texts = [fastq(N, L, 41, 1), fastq(N, L, 42, 2)]
            write(ins[0], self.texts[0])
            write(os.path.join(d, "in_2.fq"), self.texts[1])
        elif name == "il":
            a, b = cut(fastq(N, L, 41, 1)), cut(fastq(N, L, 42, 2))
            self.texts = [b"".join(x + y for x, y in zip(a, b))]
            write(ins[0], self.texts[0])
        elif name == "fa":
            self.texts = [fastq(N, L, 43, fasta=True)]
            write(ins[0], self.texts[0])
        elif name == "varlen":
            lens = np.random.default_rng(44).integers(36, L + 1, size=N)
            lens[:8] = L
            self.texts = [fastq(N, L, 45, lens=lens)]
            write(ins[0], self.texts[0])
        elif name == "two":
            self.texts = [fastq(N, L, 46)]
            recs = cut(self.texts[0])
            ins = [os.path.join(d, "ina_1.fq"), os.path.join(d, "inb_1.fq")]
            write(ins[0], b"".join(recs[:700]))
            write(ins[1], b"".join(recs[700:]))
        elif name in ("gzin", "gzmulti"):
            self.texts = [fastq(N, L, 47)]
            ins = [os.path.join(d, "in_1.fq.gz")]
            t = self.texts[0]
            third = 4 * L * (len(t) // (12 * L))
            write(ins[0], gzip.compress(t, 1) if name == "gzin" else b"".join(gzip.compress(p, 1) for p in (t[:third], t[third:2 * third + 7], t[2 * third + 7:])))
        else:
            self.texts = [fastq(N, L, 40)]
            write(ins[0], self.texts[0])
        self.ins = ins
        self.common = ["-s", "1000"] + ([] if "-c" in self.c["c"] else ["-c", "no"])
        self.logs = {}
        for out, flags in (("all", ["--lossless"]), ("dig", ["--lossless", "--digest"])):
            self.logs[out] = scalce(*self.c["c"], *self.common, *flags, "-o", os.path.join(d, out), *ins).stderr.decode()
        self.outs = 2 if name == "pe" else 1

    def arc(self, which):
        return os.path.join(self.d, which + "_1.scalcen")

    def decompress(self, which, out, *flags, ok=True, d=None):
        return scalce("-d", *(self.c["d"] if d is None else d), "-o", os.path.join(self.d, out), self.arc(which), *flags, ok=ok)

    def outputs(self, out):
        return [read(os.path.join(self.d, "%s_%d.fastq" % (out, m + 1))) for m in range(self.outs)]

    def digest(self, which="dig"):
        return fmt.unpack_digest(F.content(os.path.join(self.d, which + "_1.scalced")))

    def copy(self, to, which="dig"):
        """the archive's files under another prefix (to be tampered with); returns the new .scalcen"""
        for fn in os.listdir(self.d):
            if fn.startswith(which + "_") and ".scalce" in fn:
                write(os.path.join(self.d, to + fn[len(which):]), read(os.path.join(self.d, fn)))
        return os.path.join(self.d, to + "_1.scalcen")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory)
        return made[name]
    return get


def match_lines(log):
    return re.findall(r"Digest: (\d+) bytes, crc32 ([0-9a-f]{8}): the input's", log)


# ---- 1 and 3: the file, the other files, the check on -d, for every shape of input ---------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_digest_is_recorded_and_checked(name, cases):
    k = cases(name)
    want = [(len(t), zlib.crc32(t)) for t in k.texts]
    assert k.digest() == (KIND.get(name, 0), want)
    assert re.findall(r"Digest: (\d+) bytes, crc32 ([0-9a-f]{8})\n", k.logs["dig"]) == [(str(n), "%08x" % c) for n, c in want]
    assert "Digest" not in k.logs["all"] and not os.path.exists(os.path.join(k.d, "all_1.scalced"))
    # every other file is the one --lossless alone writes
    mine = sorted(fn for fn in os.listdir(k.d) if fn.startswith("dig_"))
    theirs = sorted(fn for fn in os.listdir(k.d) if fn.startswith("all_"))
    assert [fn[3:] for fn in mine if not fn.endswith(".scalced")] == [fn[3:] for fn in theirs] and len(mine) == len(theirs) + 1
    for fn in theirs:
        assert read(os.path.join(k.d, fn)) == read(os.path.join(k.d, "dig" + fn[3:])), fn
    if name == "gz":
        assert read(os.path.join(k.d, "dig_1.scalced"))[:2] == b"\x1f\x8b"
    if name == "gzin":  # one member: the number gzip itself keeps in the trailer, and the size next to it
        trailer = read(k.ins[0])[-8:]
        assert struct.unpack("<II", trailer) == (want[0][1], want[0][0])
    r = k.decompress("dig", "rt")
    assert k.outputs("rt") == k.texts
    assert match_lines(r.stderr.decode()) == [(str(n), "%08x" % c) for n, c in want]
    # without the stream nothing is said
    assert "Digest" not in k.decompress("all", "rt0").stderr.decode()


# ---- 2: many windows, many stripes, -S parts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "pe", "il"])
def test_many_windows_and_stripes(name, cases):
    k = cases(name)
    r = k.decompress("dig", "mw", "--window", REC * 100)
    log = r.stderr.decode()
    assert int(re.search(r"Windows: (\d+)", log).group(1)) >= 5 and int(re.search(r"through (\d+) stripes", log).group(1)) >= 3, log
    assert k.outputs("mw") == k.texts
    assert len(match_lines(log)) == len(k.texts)
    # in the archive's order each window's text is hashed, not a stripe's: the text is another, and the check says it was not made
    r = k.decompress("dig", "ao", "--archive-order", "--window", REC * 100)
    assert "Digest: not checked (--archive-order)" in r.stderr.decode()


def test_split_parts_are_still_checked(cases):
    k = cases("se")
    r = k.decompress("dig", "sp", "-S", 100, "--window", REC * 300)
    parts = [read(os.path.join(k.d, "sp.%d_1.fastq" % (i + 1))) for i in range(N // 100)]
    assert b"".join(parts) == k.texts[0]
    assert len(match_lines(r.stderr.decode())) == 1


# ---- 4 and 5: tampered archives, on -d and on -d --test -------------------------------------------------------------------------
def tampered(k, what):
    arc = k.copy("t_" + what)
    base = arc[:-len("_1.scalcen")]
    if what == "comment":   # one byte of one entry, same length
        raw = bytearray(read(base + "_1.scalcec"))
        at = raw.index(b" lane=", 24) + 6
        raw[at] = ord("9") if raw[at] != ord("9") else ord("8")
        write(base + "_1.scalcec", bytes(raw))
    elif what == "crc":
        raw = bytearray(read(base + "_1.scalced"))
        raw[32] ^= 1
        write(base + "_1.scalced", bytes(raw))
    elif what == "truncated":
        write(base + "_1.scalced", read(base + "_1.scalced")[:39])
    elif what == "magic":
        write(base + "_1.scalced", b"x" + read(base + "_1.scalced")[1:])
    elif what == "texts":   # T = 2 on a single-end archive, with its second entry
        raw = read(base + "_1.scalced")
        write(base + "_1.scalced", raw[:16] + struct.pack("<q", 2) + raw[24:] + raw[24:])
    return arc


@pytest.mark.parametrize("test_only", [False, True], ids=["d", "test"])
@pytest.mark.parametrize("what", ["comment", "crc", "truncated", "magic", "texts"])
def test_tampered_archives_end_with_status_1(what, test_only, cases, tmp_path):
    k = cases("se")
    arc = tampered(k, what)
    out = tmp_path / "outdir"
    out.mkdir()
    r = scalce("-d", *(["--test"] if test_only else ["-o", out / "x"]), arc, ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1
    n, c = len(k.texts[0]), zlib.crc32(k.texts[0])
    if what in ("comment", "crc"):
        m = re.search(r"\(ERROR\) digest mismatch in text 1: the input had (\d+) bytes, crc32 ([0-9a-f]{8}); written (\d+) bytes, crc32 ([0-9a-f]{8})", err)
        assert m, err
        if what == "comment":   # the text written is the tampered one; the record says what the input was
            assert m.group(1, 2) == (str(n), "%08x" % c) and m.group(3) == str(n) and m.group(4) != m.group(2)
            if not test_only:
                got = read(out / "x_1.fastq")
                assert len(got) == n and got != k.texts[0] and m.group(4) == "%08x" % zlib.crc32(got)   # the output stays
        else:
            assert m.group(1, 3, 4) == (str(n), str(n), "%08x" % c) and m.group(2) == "%08x" % (c ^ 1)
    else:
        assert {"truncated": "(ERROR) truncated digest stream", "magic": "is not a scalce digest stream",
                "texts": "(ERROR) digest stream holds 2 texts, the archive 1"}[what] in err
    if test_only:
        assert os.listdir(out) == []


@pytest.mark.parametrize("name", ["se", "pe", "il", "varlen"])
def test_test_writes_nothing(name, cases, tmp_path):
    k = cases(name)
    out = tmp_path / "outdir"
    out.mkdir()
    before = sorted(os.listdir(k.d))
    r = scalce("-d", *k.c["d"], "--test", "-o", out / "ignored", k.arc("dig"), "--window", REC * 300)
    assert len(match_lines(r.stderr.decode())) == len(k.texts)
    assert os.listdir(out) == [] and sorted(os.listdir(k.d)) == before
    r = scalce("-d", *k.c["d"], "--test", k.arc("all"))   # no -o at all
    assert "Digest: none recorded; streams decode to their end" in r.stderr.decode()
    assert sorted(os.listdir(k.d)) == before


# ---- 6: another text than the input's was asked for ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--archive-order"], ["--no-comments"], ["--stored-bases"], ["--bare-plus"], ["-n", "lib"],
                                   ["--records", "10:20", "--archive-order"], ["-Q"]], ids=lambda f: f[0])
def test_not_checked_when_the_text_is_not_the_inputs(flags, cases):
    k = cases("se")
    r = k.decompress("dig", "sk", *flags)
    assert re.search(r"Digest: not checked \(%s\)" % re.escape(flags[0]), r.stderr.decode()), r.stderr.decode()
    assert r.returncode == 0
    k.decompress("all", "sk0", *flags)
    assert k.outputs("sk") == k.outputs("sk0")


def test_not_checked_across_the_ways_pairs_come_in(cases):
    pe, il = cases("pe"), cases("il")
    r = pe.decompress("dig", "x", d=["-i"])
    assert "Digest: not checked (-i" in r.stderr.decode()
    r = il.decompress("dig", "x", d=["-r"])
    assert "Digest: not checked (-r" in r.stderr.decode()
    # a stream of --lossless is missing: the text is not the input's
    arc = cases("se").copy("nox")
    os.unlink(arc[:-len("_1.scalcen")] + "_1.scalcex")
    r = scalce("-d", "-o", os.path.join(cases("se").d, "nox_out"), arc)
    assert "Digest: not checked (no .scalcex)" in r.stderr.decode()


# ---- 7: refusals, before a device is touched -----------------------------------------------------------------------------------
def test_refusals(cases, tmp_path):
    k = cases("se")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no device to touch

    def refused(*args):
        r = subprocess.run([F.SCALCE, *map(str, args), "--patterns-bin", F.PBIN], capture_output=True, timeout=60, env=env)
        assert r.returncode == 1, (args, r.stderr)
        return r.stderr.decode()
    assert "(ERROR) --digest needs --lossless: only then is the text -d writes the input's" in refused("--digest", "-o", tmp_path / "a", k.ins[0])
    assert "(ERROR) --digest" in refused("--digest", "-d", "-o", tmp_path / "a", k.arc("dig"))
    assert "(ERROR) --test can be only used with decompression" in refused("--test", "-o", tmp_path / "a", k.ins[0])
    assert "(ERROR) --test" in refused("--test", "--archive-order", "-d", k.arc("dig"))
    for flags in (["--no-comments"], ["--stored-bases"], ["--bare-plus"], ["-n", "lib"], ["-Q"], ["--records", "3"]):
        assert "(ERROR) --test" in refused("--test", "-d", k.arc("dig"), *flags)
    assert os.listdir(tmp_path) == []


# ---- 8: a stale stream ----------------------------------------------------------------------------------------------------------
def test_a_run_without_the_option_removes_a_stale_stream(cases, tmp_path):
    k = cases("se")
    scalce(*k.common, "--lossless", "--digest", "-o", tmp_path / "p", k.ins[0])
    assert os.path.exists(tmp_path / "p_1.scalced")
    scalce(*k.common, "--lossless", "-o", tmp_path / "p", k.ins[0])
    assert not os.path.exists(tmp_path / "p_1.scalced")
    assert "Digest" not in scalce("-d", "-o", tmp_path / "back", tmp_path / "p_1.scalcen").stderr.decode()
    assert read(tmp_path / "back_1.fastq") == k.texts[0]
