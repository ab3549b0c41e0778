"""-m gpu: a range of records back to text (scalce -d --records FIRST[:COUNT], scalce_stream_decompress_range): the text is the
oracle's decompression of the archive, sliced by records, wherever the range lies -- on or off the window grid, on a bucket's
edge, inside a frame of the arithmetic coder, across its boundary --; what lies in front of the range is passed over and what
lies behind it is not read."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import decode_ref as R
import oraclelib as O
from scalce_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scalce_amd", "bin", "scalce")
PBIN = os.path.join(ROOT, "tests", "golden", "patterns.bin")
FRAME = R.FRAME
Q_HEADER = 16 + 4 * R.TABLE_WORDS + 8  # magic and phred offset, the table, the symbol count: the frames begin behind them


def run_cli(*args, ok=True):
    r = subprocess.run([CLI, *map(str, args), "--patterns-bin", PBIN], capture_output=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def windows_line(r):
    m = re.search(rb"\tWindows: (\d+) of up to (\d+) bytes of text; device memory held at most (\d+) bytes", r.stderr)
    assert m, r.stderr.decode(errors="replace")[-800:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def range_line(r):
    """(first, end, total or None, frames decoded, frames passed over) of the log's Range line, which follows the Windows line"""
    m = re.search(rb"\tWindows: [^\n]*\n\tRange: records (\d+) to (\d+) of (\d+|unknown); quality frames decoded (\d+), passed over (\d+)\n", r.stderr)
    assert m, r.stderr.decode(errors="replace")[-800:]
    return int(m.group(1)), int(m.group(2)), None if m.group(3) == b"unknown" else int(m.group(3)), int(m.group(4)), int(m.group(5))


def read(p):
    return open(p, "rb").read()


def records(text, lpr=4):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % lpr == 0
    return [b"\n".join(lines[i:i + lpr]) + b"\n" for i in range(0, len(lines) - 1, lpr)]


def two_line(rec):
    """what -d -Q writes for a four-line record: the name line and the bases, an N as the A it was stored as"""
    ln = rec.split(b"\n")
    return b"\n".join([ln[0], ln[1].replace(b"N", b"A")]) + b"\n"


def make_inputs(d, n, L, paired, seed):
    synth.write_fastq(str(d / "in_1.fq"), n, L, seed=seed, n_frac=0.003, dup_frac=0.1, paired_suffix="/1" if paired else None)
    if paired:
        synth.write_fastq(str(d / "in_2.fq"), n, L, seed=seed + 1, paired_suffix="/2")


def oracle_records(d, cflags, dflags, paired, stem="orc"):
    """the oracle's archive of in_1.fq (in_2.fq) and its decompression of it: per mate, the list of the records' texts"""
    O.orc_cli("compress", PBIN, d / "in_1.fq", d / stem, *cflags)
    O.orc_cli("decompress", PBIN, d / f"{stem}_1.scalcen", d / f"{stem}_back", *dflags)
    return [records(read(d / f"{stem}_back_{m}.fastq")) for m in ((1, 2) if paired else (1,))]


def cut(recs, first, count=None):
    return b"".join(recs[first:] if count is None else recs[first:first + count])


def cut_pairs(r1, r2, first, count=None):
    end = len(r1) if count is None else first + count
    return b"".join(x + y for x, y in zip(r1[first:end], r2[first:end]))


def spec(first, count):
    return f"{first}" if count is None else f"{first}:{count}"


# ---- the entry through host.py, on the files of an archive ------------------------------------------------------------------
def entry(d, stem, mates, first, count, window, skip=True, piece=None, **kw):
    """scalce_stream_decompress_range on the archive's files: (UnpackStats with .range, text per mate, first_record of every
    write).  skip: the files seek; piece: the readers hand out at most this many bytes a call."""
    from scalce_amd import host
    files = [[open(d / f"{stem}_{m}.scalce{e}", "rb") for e in "rnq"] for m in range(1, mates + 1)]

    def reader(f):
        return lambda cap: f.read(cap if piece is None else min(cap, piece))

    def skipper(f):
        def sk(n):
            pos, size = f.tell(), os.fstat(f.fileno()).st_size
            k = min(n, max(0, size - pos))
            f.seek(pos + k)
            return k
        return sk
    got, firsts = {}, []

    def write(mate, first_record, nrec, text, offs):
        firsts.append((mate, first_record, nrec))
        got.setdefault(mate, []).append(text)
    ctx = host.Context(0, patterns_bin=read(PBIN))
    try:
        st = host.stream_decompress(ctx, [[reader(f) for f in fs] for fs in files], write, mates=mates, window_text_bytes=window,
                                    first_record=first, nrecords=count, skippers=[[skipper(f) for f in fs] for fs in files] if skip else None,
                                    **kw)
    finally:
        for fs in files:
            for f in fs:
                f.close()
        ctx.close()
    return st, [b"".join(got.get(m, [])) for m in range(max(got, default=0) + 1)], firsts


def coded_frame_sizes(path):
    """the size words of a .scalceq's frames, by walking the file"""
    data = np.fromfile(path, dtype=np.uint8)
    nsym = int(data[Q_HEADER - 8:Q_HEADER].view("<u8")[0])
    sizes, pos = [], Q_HEADER
    for _ in range(-(-nsym // FRAME)):
        sizes.append(int(data[pos:pos + 4].view("<u4")[0]))
        pos += 4 + sizes[-1]
    assert pos == len(data)
    return nsym, sizes


# ---- 1: every mode, small, a range over several windows -----------------------------------------------------------------------
def bucket_edges(path, L):
    """[(first record, records, core id)] of the buckets of a plain .scalcer, by walking its headers"""
    trie = O.Trie(blob=read(PBIN))
    data = read(path)
    assert data[:7] == b"scalce2"
    pos, first, out = 16, 0, []
    while pos < len(data):
        cid, cnt = struct.unpack_from("<iQ", data, pos)
        core = b"" if cid == R.ROOT_CORE else trie.pattern(cid)
        pos += 12 + cnt * (R.sz_read(L - len(core)) + R.sz_meta(L))
        if cnt:
            out.append((first, cnt, cid))
        first += cnt
    assert pos == len(data)
    return out


@pytest.mark.parametrize("flags", [[], ["-r"], ["-A"], ["-n", "lib"], ["-c", "gz"], ["-p", "30"], ["-Q"], ["-f"], ["-i"]],
                         ids=lambda f: "_".join(f).replace("-", "") or "plain")
def test_every_mode_small(flags, tmp_path):
    d = tmp_path
    n, L = 3000, 50
    il, noq = "-i" in flags, "-Q" in flags or "-f" in flags
    paired = "-r" in flags or il
    make_inputs(d, n, L, paired, seed=131)
    # the archive: -i's is the one -r makes of the split mates; -f's the one of the FASTA form of the same records
    cflags = [f for f in flags if f != "-i"] + (["-r"] if il else [])
    src = d / "in_1.fq"
    if "-f" in flags:
        src = d / "fa_1.fa"
        src.write_bytes(b"".join(b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in records(read(d / "in_1.fq"))))
    run_cli(*(cflags if "-c" in cflags else cflags + ["-c", "no"]), "-o", d / "hip", src)
    oflags = [f for f in cflags if f not in ("-Q", "-f")]
    dflags = (["-r"] if paired else []) + (["-n", "lib"] if "-n" in flags else [])
    want = oracle_records(d, oflags, dflags, paired)
    assert all(len(w) == n for w in want)
    if noq:
        want = [[two_line(r) for r in w] for w in want]
    mine = (["-i"] if il else ["-r"] if paired else []) + (["-n", "lib"] if "-n" in flags else []) + (["-Q"] if noq else [])
    ranges = [(0, 1), (1, 1), (n - 1, 1), (n, 5), (2500, None), (2900, 500), (457, 1234)]
    if flags == []:
        # buckets of the plain read stream: a range from a bucket's first record, one from a bucket's last, one inside the root bucket
        buckets = bucket_edges(d / "hip_1.scalcer", L)
        inner = sorted((b for b in buckets if b[2] != R.ROOT_CORE and b[0] > 0), key=lambda b: -b[1])  # the largest first
        root = [b for b in buckets if b[2] == R.ROOT_CORE]
        assert len(inner) >= 2 and inner[1][1] >= 2 and len(root) == 1 and root[0][1] >= 4
        ranges += [(inner[0][0], 40), (inner[1][0] + inner[1][1] - 1, 40), (root[0][0] + 1, root[0][1] - 2)]
    coded = not noq and "-A" not in flags
    for k, (first, count) in enumerate(ranges):
        r = run_cli("-d", *mine, "--records", spec(first, count), "--window", "32K", "-o", d / f"back{k}", d / "hip_1.scalcen")
        end = n if count is None else min(n, first + count)
        if il:
            assert read(d / f"back{k}_1.fastq") == cut_pairs(want[0], want[1], first, count), (flags, first, count)
        else:
            for m, w in enumerate(want):
                assert read(d / f"back{k}_{m + 1}.fastq") == cut(w, first, count), (flags, first, count, m + 1)
        if first >= n:
            assert os.path.getsize(d / f"back{k}_1.fastq") == 0
        rl = range_line(r)
        assert rl[:2] == (min(first, n), end) and rl[2] == (n if coded else None), (flags, first, count, rl)
        if (first, count) == (457, 1234):
            assert windows_line(r)[0] >= 4 and windows_line(r)[1] == 32 << 10


# ---- 2: frames of the coder --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def archive_a(tmp_path_factory):
    """220 000 x 100 bp: three frames (104 857 records and 60 symbols each); the oracle's archive, with and without -A"""
    d = tmp_path_factory.mktemp("a")
    make_inputs(d, 220000, 100, False, seed=137)
    recs = oracle_records(d, [], [], False)[0]
    recs_raw = oracle_records(d, ["-A"], [], False, stem="raw")[0]
    assert len(recs) == len(recs_raw) == 220000
    return d, recs, recs_raw


@pytest.fixture(scope="module")
def archive_b(tmp_path_factory):
    """170 000 x 64 bp: record 163 840 begins on the second frame's first symbol"""
    d = tmp_path_factory.mktemp("b")
    make_inputs(d, 170000, 64, False, seed=139)
    return d, oracle_records(d, [], [], False)[0]


@pytest.fixture(scope="module")
def archive_c(tmp_path_factory):
    """75 000 pairs x 150 bp: in either mate record 69 905 has 10 symbols in the first frame and 140 in the second"""
    d = tmp_path_factory.mktemp("c")
    make_inputs(d, 75000, 150, True, seed=149)
    return d, oracle_records(d, ["-r"], ["-r"], True)


def check_plan(st, mate, L, first, count, total_syms, want_plan):
    from scalce_amd import host
    plan = host.range_plan_quality(L, first, count, total_syms)
    assert plan == want_plan
    rs = st.range
    assert (rs.frames_passed[mate], rs.frames_decoded[mate]) == plan[:2], (list(rs.frames_passed), list(rs.frames_decoded), plan)
    assert rs.symbols_decoded[mate] == plan[2] + plan[3], (list(rs.symbols_decoded), plan)


def test_range_inside_the_middle_frame(archive_a):
    d, recs, _ = archive_a
    st, text, firsts = entry(d, "orc", 1, 110000, 10, 2 << 20)
    assert text == [cut(recs, 110000, 10)] and firsts == [(0, 110000, 10)]
    check_plan(st, 0, 100, 110000, 10, 22000000, (1, 1, 110000 * 100 - FRAME, 1000))
    assert (st.range.first_record, st.range.nrecords, st.range.total_records) == (110000, 10, 220000)
    r = run_cli("-d", "--records", "110000:10", "--window", "2M", "-o", d / "mid", d / "orc_1.scalcen")
    assert read(d / "mid_1.fastq") == text[0] and range_line(r) == (110000, 110010, 220000, 1, 1)


def test_record_that_straddles_a_frame_boundary(archive_a):
    d, recs, _ = archive_a
    assert 104857 * 100 < FRAME < 104858 * 100
    st, text, _ = entry(d, "orc", 1, 104857, 1, 2 << 20)
    assert text == [cut(recs, 104857, 1)]
    check_plan(st, 0, 100, 104857, 1, 22000000, (0, 2, 10485700, 100))


def test_range_that_begins_on_a_frames_first_symbol(archive_b):
    d, recs = archive_b
    assert 163840 * 64 == FRAME
    st, text, _ = entry(d, "orc", 1, 163840, 10, 2 << 20)
    assert text == [cut(recs, 163840, 10)]
    check_plan(st, 0, 64, 163840, 10, 170000 * 64, (1, 1, 0, 640))


def test_range_that_ends_on_a_frames_last_symbol(archive_b):
    d, recs = archive_b
    st, text, _ = entry(d, "orc", 1, 163830, 10, 2 << 20)
    assert text == [cut(recs, 163830, 10)]
    check_plan(st, 0, 64, 163830, 10, 170000 * 64, (0, 1, 163830 * 64, 640))
    assert st.range.symbols_decoded[0] == FRAME  # the first frame to its last symbol, none of the second


@pytest.mark.parametrize("mode", ["-i", "-r"])
def test_pairs_across_each_mates_frame_boundary(mode, archive_c):
    d, (r1, r2) = archive_c
    assert 69905 * 150 < FRAME < 69906 * 150
    st, text, firsts = entry(d, "orc", 2, 69900, 10, 2 << 20, interleave=mode == "-i")
    # (a window takes whole records of one decoder batch: at one frame per batch the range is cut where the frame ends)
    if mode == "-i":
        assert text == [cut_pairs(r1, r2, 69900, 10)] and firsts == [(0, 69900, 5), (0, 69905, 5)]
    else:
        assert text == [cut(r1, 69900, 10), cut(r2, 69900, 10)]
        assert firsts == [(0, 69900, 5), (0, 69905, 5), (1, 69900, 5), (1, 69905, 5)]
    for m in (0, 1):
        check_plan(st, m, 150, 69900, 10, 75000 * 150, (0, 2, 69900 * 150, 1500))
    assert list(st.records) == [10, 10]


def test_raw_quality_rows_are_passed_over(archive_a):
    from scalce_amd import host
    d, _, recs = archive_a
    for first, count in ((110000, 10), (104857, 1)):
        st, text, firsts = entry(d, "raw", 1, first, count, 2 << 20)
        assert text == [cut(recs, first, count)] and firsts == [(0, first, count)]
        rs = st.range
        assert rs.total_records == (1 << 64) - 1 and rs.frames_decoded[0] == rs.frames_passed[0] == rs.symbols_decoded[0] == 0
        # the rows in front of the range: what the look-ahead buffer held of them, the rest through skip
        assert rs.bytes_delivered[0][2] <= 16 + host.UNPACK_LOOKAHEAD_BYTES + count * 100
        assert first * 100 - host.UNPACK_LOOKAHEAD_BYTES <= rs.bytes_skipped[0][2] <= first * 100
    r = run_cli("-d", "--records", "110000:10", "--window", "2M", "-o", d / "rawmid", d / "raw_1.scalcen")
    assert read(d / "rawmid_1.fastq") == cut(recs, 110000, 10) and range_line(r) == (110000, 110010, None, 0, 0)


# ---- 3: slices make the whole ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "il", "nlib"])
def test_slices_make_the_whole(mode, tmp_path):
    d = tmp_path
    n, il = 3000, mode == "il"
    make_inputs(d, n, 50, il, seed=151)
    fl = (["-r"] if il else []) + (["-n", "lib"] if mode == "nlib" else [])
    want = oracle_records(d, fl, fl, il)
    whole = cut_pairs(want[0], want[1], 0) if il else cut(want[0], 0)
    rng = np.random.default_rng(157)
    cuts = sorted({0, n, *map(int, rng.integers(1, n, size=3))})
    assert len(cuts) == 5
    parts = []
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        run_cli("-d", *(["-i"] if il else []), *fl[1 if il else 0:], "--records", f"{a}:{b - a}", "--window", "32K", "-o", d / f"s{k}", d / "orc_1.scalcen")
        parts.append(read(d / f"s{k}_1.fastq"))
        assert parts[-1].count(b"\n") == (8 if il else 4) * (b - a)
    assert b"".join(parts) == whole


def test_split_parts_count_from_the_ranges_first_record(tmp_path):
    d = tmp_path
    make_inputs(d, 3000, 50, False, seed=163)
    recs = oracle_records(d, [], [], False)[0]
    r = run_cli("-d", "--records", "457:1234", "-S", "500", "--window", "32K", "-o", d / "part", d / "orc_1.scalcen")
    for k, (a, c) in enumerate([(457, 500), (957, 500), (1457, 234)]):
        assert read(d / f"part.{k + 1}_1.fastq") == cut(recs, a, c), k + 1
    assert not os.path.exists(d / "part.4_1.fastq")
    made = re.findall(rb"Created (\S+) with (\d+) reads", r.stderr)
    assert [(os.path.basename(f.decode()), int(c)) for f, c in made] == [("part.1_1.fastq", 500), ("part.2_1.fastq", 500), ("part.3_1.fastq", 234)]
    assert range_line(r)[:3] == (457, 1691, 3000)


# ---- 4: the index of made-up names stays the archive's ---------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 0], ids=["one_record_per_window", "default_window"])
def test_library_index_is_archive_absolute(window, tmp_path):
    d = tmp_path
    n = 1100
    make_inputs(d, n, 50, False, seed=167)
    recs = oracle_records(d, ["-n", "lib"], ["-n", "lib"], False)[0]
    assert recs[999].startswith(b"@lib.999\n") and recs[1000].startswith(b"@lib.1000\n")
    for first in (9, 10, 99, 100, 999):
        st, text, firsts = entry(d, "orc", 1, first, 3, window, library="lib")
        assert text == [cut(recs, first, 3)], first
        assert text[0].startswith(b"@lib.%d\n" % first)
        assert firsts == ([(0, first + k, 1) for k in range(3)] if window else [(0, first, 3)])


# ---- 5: -o - ---------------------------------------------------------------------------------------------------------------------
def test_stdout_gets_the_range(tmp_path):
    d = tmp_path
    make_inputs(d, 3000, 50, True, seed=173)
    recs = oracle_records(d, [], [], False)[0]
    r = run_cli("-d", "--records", "457:1234", "--window", "32K", "-o", "-", d / "orc_1.scalcen")
    assert r.stdout == cut(recs, 457, 1234) and range_line(r)[:3] == (457, 1691, 3000)
    O.orc_cli("compress", PBIN, d / "in_1.fq", d / "pe", "-r")
    r = run_cli("-d", "-r", "--records", "457:1234", "-o", "-", d / "pe_1.scalcen", ok=False)
    assert r.returncode != 0 and b"stdout can be only used with single-end" in r.stderr and r.stdout == b""


# ---- 6: truncation in front of, inside and behind the range ------------------------------------------------------------------
def test_truncation_behind_the_range_is_not_noticed(archive_a, tmp_path):
    a, recs, _ = archive_a
    d = tmp_path
    nsym, sizes = coded_frame_sizes(a / "orc_1.scalceq")
    assert len(sizes) == 3 and sizes[2] > 2000
    for e in "rnq":
        shutil.copy(a / f"orc_1.scalce{e}", d / f"qcut_1.scalce{e}")
        shutil.copy(a / f"orc_1.scalce{e}", d / f"ncut_1.scalce{e}")
    with open(d / "qcut_1.scalceq", "r+b") as f:  # inside the last frame
        f.truncate(os.path.getsize(d / "qcut_1.scalceq") - 1000)
    names = read(a / "orc_1.scalcen")
    with open(d / "ncut_1.scalcen", "r+b") as f:  # inside a name of the archive's second half
        f.truncate(len(names) * 3 // 4)
    for stem in ("qcut", "ncut"):
        r = run_cli("-d", "--records", "10:5", "--window", "2M", "-o", d / f"{stem}_ok", d / f"{stem}_1.scalcen")
        assert read(d / f"{stem}_ok_1.fastq") == cut(recs, 10, 5)
        assert range_line(r) == (10, 15, 220000, 1, 0)
    r = run_cli("-d", "--records", "219990:5", "--window", "2M", "-o", d / "qcut_bad", d / "qcut_1.scalcen", ok=False)
    assert r.returncode == 1 and b"(ERROR) truncated quality stream" in r.stderr, r.stderr[-300:]
    r = run_cli("-d", "--records", "219990:5", "--window", "2M", "-o", d / "ncut_bad", d / "ncut_1.scalcen", ok=False)
    assert r.returncode == 1 and b"(ERROR) truncated name stream" in r.stderr, r.stderr[-300:]


# ---- 7: the entry itself -----------------------------------------------------------------------------------------------------------
def test_entry_with_small_pieces_with_and_without_skippers(tmp_path):
    d = tmp_path
    n = 3000
    make_inputs(d, n, 50, True, seed=179)
    r1, r2 = oracle_records(d, ["-r"], ["-r"], True)
    for piece, skip in ((4093, True), (4093, False), (7, True), (61, False)):
        st, text, firsts = entry(d, "orc", 2, 457, 1234, 32 << 10, skip=skip, piece=piece)
        assert text == [cut(r1, 457, 1234), cut(r2, 457, 1234)], (piece, skip)
        # first_record of every window is the archive's, windows follow each other, mate 1 then mate 2
        for m in (0, 1):
            w = [(f, k) for mate, f, k in firsts if mate == m]
            assert w[0][0] == 457 and all(a[0] + a[1] == b[0] for a, b in zip(w, w[1:])) and w[-1][0] + w[-1][1] == 1691 and len(w) >= 4
        assert [mate for mate, _, _ in firsts] == sorted(mate for mate, _, _ in firsts)
        rs = st.range
        assert (rs.first_record, rs.nrecords, rs.total_records) == (457, 1234, n) and list(st.records) == [1234, 1234]
        skipped = sum(rs.bytes_skipped[m][k] for m in (0, 1) for k in (0, 1, 2))
        # mate 2's read stream alone passes over 457 x 13 bytes, more than the look-ahead buffer holds after one piece
        assert (skipped > 0) == skip, (piece, skip, skipped)
    st, text, firsts = entry(d, "orc", 2, n + 7, 5, 32 << 10, interleave=True)
    assert text == [b""] and firsts == [] and (st.range.first_record, st.range.nrecords) == (n, 0)
    st, text, _ = entry(d, "orc", 2, 2990, 500, 32 << 10, interleave=True)
    assert text == [cut_pairs(r1, r2, 2990)] and (st.range.first_record, st.range.nrecords) == (2990, 10)


def test_entry_reads_the_frames_it_decodes_and_no_others(archive_a):
    from scalce_amd import host
    d, recs, _ = archive_a
    nsym, sizes = coded_frame_sizes(d / "orc_1.scalceq")
    assert nsym == 22000000 and len(sizes) == 3
    whole, text_whole, _ = entry(d, "orc", 1, 0, None, 2 << 20)
    assert text_whole == [cut(recs, 0)]
    st, text, _ = entry(d, "orc", 1, 110000, 10, 2 << 20)
    assert text == [cut(recs, 110000, 10)]
    rs = st.range
    assert (rs.frames_passed[0], rs.frames_decoded[0]) == (1, 1)
    # from the design, not a measurement: header, table and symbol count, the coded bytes of the frame that is decoded, a size
    # word per frame passed over, and what the look-ahead buffer may hold beyond what was asked for
    bound = Q_HEADER + sizes[1] + 4 * 1 + host.UNPACK_LOOKAHEAD_BYTES
    print("quality bytes delivered", rs.bytes_delivered[0][2], "bound", bound, "file", os.path.getsize(d / "orc_1.scalceq"))
    assert rs.bytes_delivered[0][2] <= bound <= os.path.getsize(d / "orc_1.scalceq") - sizes[0] + host.UNPACK_LOOKAHEAD_BYTES
    assert rs.bytes_skipped[0][2] >= sizes[0] - host.UNPACK_LOOKAHEAD_BYTES
    assert whole.range.bytes_delivered[0][2] == os.path.getsize(d / "orc_1.scalceq") and list(whole.range.frames_decoded) == [3, 0]
    assert 0 < st.peak_device_bytes <= whole.peak_device_bytes and st.window_text_bytes == whole.window_text_bytes == 2 << 20


# ---- 8: the flag's errors ------------------------------------------------------------------------------------------------------------
def test_records_flag_errors(tmp_path):
    d = tmp_path
    make_inputs(d, 100, 50, False, seed=181)
    r = run_cli("--records", "5", "-c", "no", "-o", d / "x", d / "in_1.fq", ok=False)
    assert r.returncode == 1 and b"--records" in r.stderr and not os.path.exists(d / "x_1.scalcen")
    run_cli("-c", "no", "-o", d / "a", d / "in_1.fq")
    for bad in ("x", "5:", "-1", "1:2:3"):
        r = run_cli("-d", "--records", bad, "-o", d / "y", d / "a_1.scalcen", ok=False)
        assert r.returncode == 1 and b"--records takes FIRST or FIRST:COUNT" in r.stderr, (bad, r.stderr[-300:])
        assert not os.path.exists(d / "y_1.fastq")
    r = run_cli("-d", "--records", "5:3", "-o", d / "y", d / "a_1.scalcen")
    assert read(d / "y_1.fastq").count(b"\n") == 12
