"""-m gpu: `scalce --variable-length` as a program.

Against the reference: the .scalcer, .scalcen and .scalceq of a variable-length run are byte for byte what the reference's own
compress() (oracle/_ref/ref_full) writes for the same records padded with N to L, and its decompress() reads our archive.
Round trip: `scalce -d` writes what the reference restores, each record cut to its true length, looked up by its name.
Then the refusals, the errors of a damaged .scalcel, and that fixed-length input is left alone."""
import os
import subprocess

import numpy as np
import pytest

import filecases as F
import varlen_util as V
from scalce_amd import format as FMT

pytestmark = pytest.mark.gpu
have_ref = pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")


def scalce(*args, ok=True):
    r = subprocess.run([F.SCALCE, *map(str, args), "--patterns-bin", F.PBIN], capture_output=True, timeout=600)
    if ok is not None:
        assert (r.returncode == 0) == ok, (args, r.returncode, r.stderr[-1500:])
    return r


def ref(mode, *args):
    r = subprocess.run([F.REF_FULL, mode, F.PBIN, *map(str, args), "-T", "1"], capture_output=True, timeout=600)
    assert r.returncode == 0, (mode, args, r.stderr[-1500:])


def read(p):
    return open(p, "rb").read()


def write(p, data):
    with open(p, "wb") as f:
        f.write(data)
    return str(p)


def archive(d, stem, m=1):
    return {ext: F.content(os.path.join(str(d), "%s_%d.scalce%s" % (stem, m, ext))) for ext in "rnq"}


# flags in the reference's spelling (-B in bytes) and ours
CASES = {
    "se100": dict(n=1200, L=(100,), ref=[], ours=[]),
    "pe150_120": dict(n=700, L=(150, 120), ref=["-r"], ours=["-r"]),
    "se100_B": dict(n=13000, L=(100,), ref=["-B", "1048576"], ours=["-B", "1M"], chunks=2),
    "se100_A": dict(n=800, L=(100,), ref=["-A"], ours=["-A"]),
    "se100_nlib": dict(n=800, L=(100,), ref=["-n", "lib"], ours=["-n", "lib"]),
    # the first 500 records are full length: both tools sample the same characters, so the lossy maps agree
    "se100_p30_s500": dict(n=1500, L=(100,), ref=["-p", "30", "-s", "500"], ours=["-p", "30", "-s", "500"], full=500),
    "se100_gz": dict(n=800, L=(100,), ref=["-c", "gz"], ours=["-c", "gz"]),
}


def make_case(name, d):
    """inputs of a case in directory d: var_<m>.fq and pad_<m>.fq; returns per mate (lens, names, var text, padded text)"""
    c = CASES[name]
    mates = []
    for m, L in enumerate(c["L"]):
        lens = V.lengths_covering(c["n"], L, 100 + m)
        lens[:c.get("full", 0)] = L
        kw = dict(prefix="p.", suffix="/%d" % (m + 1)) if len(c["L"]) == 2 else {}
        var, pad, names = V.texts(L, lens, 200 + m, **kw)
        write(os.path.join(str(d), "var_%d.fq" % (m + 1)), var)
        write(os.path.join(str(d), "pad_%d.fq" % (m + 1)), pad)
        mates.append((lens, names, var, pad))
    return mates


def compress_both(name, d, with_ref=True):
    c = CASES[name]
    d = str(d)
    ours = c["ours"] + ([] if "-c" in c["ours"] else ["-c", "no"])
    r = scalce("--variable-length", *ours, "-o", os.path.join(d, "ours"), os.path.join(d, "var_1.fq"))
    if with_ref:
        ref("compress", os.path.join(d, "pad_1.fq"), os.path.join(d, "ref"), *c["ref"], "-t", os.path.join(d, "tmp_ref"))
    return r


@have_ref
@pytest.mark.parametrize("name", list(CASES))
def test_archive_is_the_references_of_the_padded_text(name, tmp_path):
    c = CASES[name]
    mates = make_case(name, tmp_path)
    r = compress_both(name, tmp_path)
    if "chunks" in c:
        line = next(ln for ln in r.stderr.decode().splitlines() if "Spill chunks" in ln)
        assert int(line.split("Spill chunks:")[1].split(",")[0]) >= c["chunks"], line
    for m in range(len(c["L"])):
        ours, theirs = archive(tmp_path, "ours", m + 1), archive(tmp_path, "ref", m + 1)
        for ext in "rnq":
            assert ours[ext] == theirs[ext], "%s: .scalce%s of mate %d" % (name, ext, m + 1)
    # the reference reads our archive: every read comes back padded, in archive order -- which is also what .scalcel follows
    ref("decompress", tmp_path / "ours_1.scalcen", tmp_path / "back", *(["-r"] if len(c["L"]) == 2 else []))
    ref("decompress", tmp_path / "ref_1.scalcen", tmp_path / "rback", *(["-r"] if len(c["L"]) == 2 else []))
    for m, (lens, names, var, pad) in enumerate(mates):
        L = c["L"][m]
        back = read(tmp_path / ("back_%d.fastq" % (m + 1)))
        assert back == read(tmp_path / ("rback_%d.fastq" % (m + 1)))
        recs = V.records_of(back)
        assert len(recs) == len(lens)
        stored_L, entries = FMT.unpack_lengths(F.content(str(tmp_path / ("ours_%d.scalcel" % (m + 1)))))
        assert stored_L == L and len(entries) == len(lens)
        if "-n" in c["ours"]:
            assert sorted(entries) == sorted(L - lens)   # (made-up names: nothing to look a record up by)
            continue
        # (lossy: qualities are not the input's, and a base whose quality maps to the offset comes back as N; the reference's
        # archive above pins both)
        lossy = "-p" in c["ours"]
        padded = {r_[:r_.index(b"\n")]: r_ for r_ in V.records_of(pad)}
        length_of = dict(zip(names, lens))
        for k, rec in enumerate(recs):
            name_line, seq, plus, qual = rec[:-1].split(b"\n")
            want = padded[name_line]   # (mate 2: mate 1's stored name with the mate's digit, which is its own)
            wn, wseq, _, wqual = want[:-1].split(b"\n")
            assert lossy or seq == wseq, "record %d" % k
            # (the quality under an N comes back as the offset character, qualities.cpp:183)
            assert lossy or qual == bytes(33 if b == 78 else q for b, q in zip(wseq, wqual)), "record %d" % k
            assert entries[k] == L - length_of[wn[1:]], "entry %d of the length stream" % k


# ---- round trip ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se(tmp_path_factory):
    """a single-end archive of ours, and what `scalce -d` must write for it: the reference's decompress() of it, every record cut
    to its true length"""
    d = tmp_path_factory.mktemp("varlen_se")
    (lens, names, var, pad), = make_case("se100", d)
    compress_both("se100", d, with_ref=False)
    ref("decompress", d / "ours_1.scalcen", d / "back")
    want = V.cut_to_lengths(read(d / "back_1.fastq"), dict(zip(names, lens)))
    assert sorted(V.records_of(want)) != sorted(V.records_of(pad)) and len(want) < len(pad)
    return dict(d=d, lens=lens, names=names, want=want, recs=V.records_of(want), n=len(lens), padded_bytes=len(pad))


@have_ref
@pytest.mark.parametrize("window", [None, 1, "three"], ids=["default", "one_record_per_window", "three_windows"])
def test_round_trip_windows(window, se):
    d = se["d"]
    # (windows are sized by the padded text: a third of it and a little more makes three)
    w = [] if window is None else ["--window", 1 if window == 1 else se["padded_bytes"] // 3 + 400]
    r = scalce("-d", "-o", d / ("rt_%s" % window), d / "ours_1.scalcen", *w)
    assert read(d / ("rt_%s_1.fastq" % window)) == se["want"]
    nwin = int(next(ln for ln in r.stderr.decode().splitlines() if "Windows:" in ln).split("Windows:")[1].split()[0])
    assert nwin == {None: 1, 1: se["n"], "three": 3}[window]


@have_ref
def test_round_trip_split_across_a_window_boundary(se):
    d, n = se["d"], se["n"]
    per = 350   # parts of 350 records, windows of about 400: parts begin and end inside windows
    scalce("-d", "-S", per, "--window", 206 * 400, "-o", d / "sp", d / "ours_1.scalcen")
    parts = [read(d / ("sp.%d_1.fastq" % (k + 1))) for k in range((n + per - 1) // per)]
    assert [len(V.records_of(p)) for p in parts] == [per] * (n // per) + ([n % per] if n % per else [])
    assert b"".join(parts) == se["want"]


@have_ref
def test_round_trip_to_stdout(se):
    r = scalce("-d", "-o", "-", se["d"] / "ours_1.scalcen", "--window", 206 * 500)
    assert r.stdout == se["want"]


@have_ref
def test_round_trip_record_ranges(se):
    d, n, recs = se["d"], se["n"], se["recs"]
    for K in (0, 1, n - 1, n):
        scalce("-d", "--records", "%d:%d" % (K, 2 * n), "--window", "1M", "-o", d / ("rg%d" % K), d / "ours_1.scalcen")
        assert read(d / ("rg%d_1.fastq" % K)) == b"".join(recs[K:]), "from record %d to the end" % K
    slices = []
    for a, cnt in ((0, 1), (1, 499), (500, n - 501), (n - 1, 5)):
        scalce("-d", "--records", "%d:%d" % (a, cnt), "--window", 206 * 300, "-o", d / ("sl%d" % a), d / "ours_1.scalcen")
        slices.append(read(d / ("sl%d_1.fastq" % a)))
    assert b"".join(slices) == se["want"]


@have_ref
def test_round_trip_paired_and_gzip_container(tmp_path):
    mates = make_case("pe150_120", tmp_path)
    scalce("--variable-length", "-r", "-c", "gz", "-o", tmp_path / "ours", tmp_path / "var_1.fq")
    assert read(tmp_path / "ours_1.scalcel")[:2] == b"\x1f\x8b" and read(tmp_path / "ours_2.scalcel")[:2] == b"\x1f\x8b"
    ref("decompress", tmp_path / "ours_1.scalcen", tmp_path / "back", "-r")
    scalce("-d", "-r", "-o", tmp_path / "rt", tmp_path / "ours_1.scalcen", "--window", 300 * 250)
    scalce("-d", "-r", "--records", "123:400", "--window", "1M", "-o", tmp_path / "rg", tmp_path / "ours_1.scalcen")
    for m, (lens, names, var, pad) in enumerate(mates):
        # (the archive keeps mate 1's names; mate 2's come back with its digit)
        want = V.cut_to_lengths(read(tmp_path / ("back_%d.fastq" % (m + 1))), dict(zip(names, lens)))
        assert read(tmp_path / ("rt_%d.fastq" % (m + 1))) == want
        assert read(tmp_path / ("rg_%d.fastq" % (m + 1))) == b"".join(V.records_of(want)[123:523])
        assert sorted(V.records_of(want)) == sorted(V.records_of(V.cut_to_lengths(_n_quality(pad), dict(zip(names, lens)))))


def _n_quality(text):
    """a text as the archive restores it: the quality under an N is the offset character"""
    out = []
    for rec in V.records_of(text):
        name, seq, plus, qual = rec[:-1].split(b"\n")
        out.append(name + b"\n" + seq + b"\n" + plus + b"\n" + bytes(33 if b == 78 else q for b, q in zip(seq, qual)) + b"\n")
    return b"".join(out)


def test_round_trip_without_the_reference(se_plain):
    """the same round trip held against the input itself: the records of the variable text, the quality under an N being the
    offset character, in the order of the archive's names"""
    d, want = se_plain
    scalce("-d", "-o", d / "rt", d / "ours_1.scalcen", "--window", 206 * 333)
    got = V.records_of(read(d / "rt_1.fastq"))
    assert sorted(got) == sorted(V.records_of(want)) and len(got) == len(set(got))


@pytest.fixture(scope="module")
def se_plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("varlen_plain")
    (lens, names, var, pad), = make_case("se100", d)
    compress_both("se100", d, with_ref=False)
    return d, _n_quality(var)


# ---- refusals and errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(["-i"], "-i"), (["-f"], "-f"), (["-Q"], "-Q"), (["--gpus", "2"], "--gpus")])
def test_compress_refuses_the_flag_with(flags, word, tmp_path):
    make_case("se100_A", tmp_path)
    r = scalce("--variable-length", *flags, "-c", "no", "-o", tmp_path / "x", tmp_path / "var_1.fq", ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1 and "(ERROR)" in err and "--variable-length" in err and word in err
    assert not os.path.exists(tmp_path / "x_1.scalcer")


@pytest.mark.parametrize("flags", [["-i"], ["-Q"]])
def test_decompress_refuses_a_length_stream_with(flags, se_plain, tmp_path):
    d, _ = se_plain
    r = scalce("-d", *flags, "-o", tmp_path / "x", d / "ours_1.scalcen", ok=False)
    assert r.returncode == 1 and "(ERROR)" in r.stderr.decode() and "variable-length" in r.stderr.decode()


def damaged(se_plain, tmp_path, change):
    d, _ = se_plain
    for ext in "rnql":
        data = read(d / ("ours_1.scalce%s" % ext))
        write(tmp_path / ("a_1.scalce%s" % ext), change(data) if ext == "l" else data)
    return tmp_path / "a_1.scalcen"


def test_length_stream_cut_short(se_plain, tmp_path):
    n = CASES["se100"]["n"]
    # at a window boundary (a record per window), inside a window (one window holds the archive), one entry short of the
    # records, inside the header
    for k, (keep, window) in enumerate(((16 + 400, 1), (16 + 400, "1M"), (16 + n - 1, "1M"), (15, "1M"))):
        arc = damaged(se_plain, tmp_path, lambda data: data[:keep])
        r = scalce("-d", "-o", tmp_path / ("o%d" % k), arc, *(["--window", window] if window else []), ok=False)
        assert r.returncode == 1 and "(ERROR) truncated length stream" in r.stderr.decode(), (keep, window, r.stderr[-400:])


def test_length_stream_cut_inside_an_entry(tmp_path):
    """two-byte entries (L = 300): the stream ends in the middle of one"""
    lens = V.lengths_covering(400, 300, 7)
    var, _, _ = V.texts(300, lens, 8)
    scalce("--variable-length", "-c", "no", "-o", tmp_path / "w", write(tmp_path / "w_1.fq", var))
    data = read(tmp_path / "w_1.scalcel")
    assert len(data) == 16 + 2 * 400
    write(tmp_path / "w_1.scalcel", data[:16 + 2 * 250 + 1])
    r = scalce("-d", "-o", tmp_path / "o", tmp_path / "w_1.scalcen", "--window", 606 * 100, ok=False)
    assert r.returncode == 1 and "(ERROR) truncated length stream" in r.stderr.decode()


def test_length_stream_for_another_read_length(se_plain, tmp_path):
    arc = damaged(se_plain, tmp_path, lambda data: data[:12] + (99).to_bytes(4, "little") + data[16:])
    r = scalce("-d", "--window", "1M", "-o", tmp_path / "o", arc, ok=False)
    assert r.returncode == 1 and "(ERROR)" in r.stderr.decode() and "99" in r.stderr.decode()


def test_without_its_length_stream_an_archive_decodes_to_padded_reads(se_plain, tmp_path):
    d, want = se_plain
    for ext in "rnq":
        write(tmp_path / ("a_1.scalce%s" % ext), read(d / ("ours_1.scalce%s" % ext)))
    scalce("-d", "--window", "1M", "-o", tmp_path / "o", tmp_path / "a_1.scalcen")
    got = V.records_of(read(tmp_path / "o_1.fastq"))
    pad = V.records_of(_n_quality(read(d / "pad_1.fq")))
    assert sorted(got) == sorted(pad)


# ---- fixed-length input is left alone -----------------------------------------------------------------------------------------
def test_fixed_length_input_gives_the_same_archive_with_and_without_the_flag(tmp_path):
    var, pad, _ = V.texts(100, np.full(900, 100), 9)
    assert var == pad
    src = write(tmp_path / "in_1.fq", var)
    scalce("-c", "no", "-o", tmp_path / "plain", src)
    scalce("--variable-length", "-c", "no", "-o", tmp_path / "flag", src)
    assert archive(tmp_path, "plain") == archive(tmp_path, "flag")
    assert not os.path.exists(tmp_path / "plain_1.scalcel")
    L, entries = FMT.unpack_lengths(read(tmp_path / "flag_1.scalcel"))
    assert L == 100 and len(entries) == 900 and not entries.any()


def test_a_length_mismatch_without_the_flag_fails_as_before(tmp_path):
    var, _, _ = V.texts(100, V.lengths_covering(300, 100, 10), 11)
    r = scalce("-c", "no", "-o", tmp_path / "x", write(tmp_path / "in_1.fq", var), ok=False)
    assert r.returncode == 1 and "read or quality line length differs from read_length" in r.stderr.decode()
    assert not os.path.exists(tmp_path / "x_1.scalcel")


def test_max_length_sets_L_and_a_longer_read_is_the_error(tmp_path):
    lens = V.lengths_covering(300, 80, 12)
    var, _, _ = V.texts(80, lens, 13)
    src = write(tmp_path / "in_1.fq", var)
    scalce("--max-length", 120, "-c", "no", "-o", tmp_path / "m", src)   # implies --variable-length
    L, entries = FMT.unpack_lengths(read(tmp_path / "m_1.scalcel"))
    assert L == 120 and sorted(entries) == sorted(120 - lens) and read(tmp_path / "m_1.scalcer")[12:16] == (120).to_bytes(4, "little")
    r = scalce("--max-length", 60, "-c", "no", "-o", tmp_path / "s", src, ok=False)
    assert r.returncode == 1 and "--max-length" in r.stderr.decode() and "(ERROR) record" in r.stderr.decode()
