"""-m gpu: decompression in windows of whole records (scalce -d --window, scalce_stream_decompress): however the windows
fall -- several per frame of the arithmetic coder, a frame boundary inside a record, a window that is one record and a whole
bucket, -S parts across windows -- the text is the oracle's, and memory follows the window, not the archive."""
import os
import re
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


def run_cli(*args, ok=True):
    r = subprocess.run([CLI, *map(str, args), "--patterns-bin", PBIN], capture_output=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def windows_line(r):
    m = re.search(rb"\tWindows: (\d+) of up to (\d+) bytes of text; device memory held at most (\d+) bytes", r.stderr)
    assert m, r.stderr.decode(errors="replace")[-800:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def read(p):
    return open(p, "rb").read()


def records(text, lpr=4):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % lpr == 0
    return [b"\n".join(lines[i:i + lpr]) + b"\n" for i in range(0, len(lines) - 1, lpr)]


def interleaved(t1, t2, lpr=4):
    a, b = records(t1, lpr), records(t2, lpr)
    assert len(a) == len(b)
    return b"".join(x + y for x, y in zip(a, b))


def two_line(text):
    """what -d -Q writes for the records of a four-line text: the name line and the bases, an N as the A it was stored as"""
    return b"".join(b"\n".join([ln[0], ln[1].replace(b"N", b"A")]) + b"\n" for ln in (r.split(b"\n") for r in records(text)))


def make_inputs(d, n, L, paired, seed=31):
    synth.write_fastq(str(d / "in_1.fq"), n, L, seed=seed, n_frac=0.003, dup_frac=0.1, paired_suffix="/1" if paired else None)
    if paired:
        synth.write_fastq(str(d / "in_2.fq"), n, L, seed=seed + 1, paired_suffix="/2")


def oracle_text(d, cflags, dflags, paired):
    """the oracle's archive of in_1.fq (in_2.fq) and its decompression of it: the FASTQ text per mate"""
    O.orc_cli("compress", PBIN, d / "in_1.fq", d / "orc", *cflags)
    O.orc_cli("decompress", PBIN, d / "orc_1.scalcen", d / "oback", *dflags)
    return [read(d / f"oback_{m}.fastq") for m in ((1, 2) if paired else (1,))]


# ---- 1: every mode, several windows per frame ----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-r"], ["-A"], ["-n", "lib"], ["-c", "gz"], ["-p", "30"], ["-Q"], ["-f"], ["-i"],
                                   ["-r", "-c", "gz", "-p", "10"]], ids=lambda f: "_".join(f).replace("-", "") or "plain")
def test_every_mode_in_several_windows(flags, tmp_path):
    d = tmp_path
    n, L = 8000, 100
    il, noq = "-i" in flags, "-Q" in flags or "-f" in flags
    paired = "-r" in flags or il
    make_inputs(d, n, L, paired)
    # the archive: -i's is the one -r makes of the split mates; -f's the one of the FASTA form of the same records
    cflags = [f for f in flags if f != "-i"] + (["-r"] if il else [])
    src = d / "in_1.fq"
    if "-f" in flags:
        src = d / "fa_1.fa"
        src.write_bytes(b"".join(b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in records(read(d / "in_1.fq"))))
    run_cli(*(cflags if "-c" in cflags else cflags + ["-c", "no"]), "-o", d / "hip", src)
    oflags = [f for f in cflags if f not in ("-Q", "-f")]
    dflags = (["-r"] if paired else []) + (["-n", "lib"] if "-n" in flags else [])
    want = oracle_text(d, oflags, dflags, paired)
    if noq:
        want = [two_line(t) for t in want]
    if il:
        want = [interleaved(want[0], want[1])]
    mine = (["-i"] if il else ["-r"] if paired else []) + (["-n", "lib"] if "-n" in flags else []) + (["-Q"] if noq else [])
    r = run_cli("-d", *mine, "--window", "256K", "-o", d / "back", d / "hip_1.scalcen")
    for m, w in enumerate(want):
        assert read(d / f"back_{m + 1}.fastq") == w, f"{flags} mate {m + 1}"
    assert windows_line(r)[0] >= 6 and windows_line(r)[1] == 256 << 10


# ---- 2: a frame boundary inside a record -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,paired", [(110000, 100, False), (75000, 150, True)], ids=["se100_two_frames", "pe150_two_frames"])
def test_frame_boundary_inside_a_record(n, L, paired, tmp_path):
    """10 485 760 symbols per frame: 104 857 x 100 + 60, and 69 905 x 150 + 10 -- a record with symbols in both frames"""
    d = tmp_path
    assert n * L > 10485760 and 10485760 % L
    make_inputs(d, n, L, paired, seed=47)
    fl = ["-r"] if paired else []
    want = oracle_text(d, fl, fl, paired)
    r = run_cli("-d", *fl, "--window", "4M", "-o", d / "back", d / "orc_1.scalcen")
    for m, w in enumerate(want):
        assert read(d / f"back_{m + 1}.fastq") == w, f"mate {m + 1}"
    assert windows_line(r)[0] >= 5


# ---- 3: every alignment of window and bucket ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "nlib", "il"])
def test_one_record_per_window(mode, tmp_path):
    """--window 1: a window starts at, ends at and is a whole bucket, root-bucket records come last; with made-up names the
    index gains a digit at window edges (9 -> 10, 99 -> 100, 999 -> 1000)"""
    d = tmp_path
    il = mode == "il"
    n = 550 if il else 1100
    make_inputs(d, n, 100, il, seed=53)
    fl = (["-r"] if il else []) + (["-n", "lib"] if mode == "nlib" else [])
    want = oracle_text(d, fl, fl, il)
    if il:
        want = [interleaved(*want)]
    r = run_cli("-d", *(["-i"] if il else []), *fl[1 if il else 0:], "--window", "1", "-o", d / "back", d / "orc_1.scalcen")
    assert read(d / "back_1.fastq") == want[0]
    assert windows_line(r)[0] == n


def test_library_index_gains_a_digit_inside_a_window(tmp_path):
    d = tmp_path
    make_inputs(d, 12000, 100, False, seed=59)
    want = oracle_text(d, ["-n", "lib"], ["-n", "lib"], False)
    r = run_cli("-d", "-n", "lib", "--window", "64K", "-o", d / "back", d / "orc_1.scalcen")
    assert read(d / "back_1.fastq") == want[0]
    assert b"@lib.9999\n" in want[0] and b"@lib.10000\n" in want[0] and windows_line(r)[0] > 30


# ---- 4: -S across windows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [False, True], ids=["reads", "pairs"])
def test_split_parts_across_windows(il, tmp_path):
    d = tmp_path
    n = 5000
    make_inputs(d, n, 100, il, seed=61)
    fl = ["-r"] if il else []
    want = oracle_text(d, fl, fl, il)
    whole = interleaved(*want) if il else want[0]
    r = run_cli("-d", *(["-i"] if il else []), "-S", "1500", "--window", "200K", "-o", d / "part", d / "orc_1.scalcen")
    parts = [read(d / f"part.{k}_1.fastq") for k in (1, 2, 3, 4)]
    assert [p.count(b"\n") // (8 if il else 4) for p in parts] == [1500, 1500, 1500, 500]
    assert b"".join(parts) == whole and not os.path.exists(d / "part.5_1.fastq")
    assert windows_line(r)[0] >= 6


# ---- 5: memory does not follow the archive -------------------------------------------------------------------------------
def test_memory_follows_the_window_not_the_archive(tmp_path):
    peak = {}
    for n in (110000, 220000):
        d = tmp_path / str(n)
        d.mkdir()
        make_inputs(d, n, 100, False, seed=67)
        want = oracle_text(d, [], [], False)
        r = run_cli("-d", "--window", "2M", "-o", d / "back", d / "orc_1.scalcen")
        assert read(d / "back_1.fastq") == want[0], n
        peak[n] = windows_line(r)[2]
    print("peak device bytes:", peak)
    assert peak[220000] <= peak[110000] + (1 << 20), peak


# ---- 6: truncation under windows ---------------------------------------------------------------------------------------
def test_truncated_streams_are_found_in_their_window(tmp_path):
    d = tmp_path
    make_inputs(d, 20000, 100, False, seed=43)
    run_cli("-c", "no", "-o", d / "a", d / "in_1.fq")
    for ext, cut in (("r", 11), ("n", 7), ("q", 5)):
        for e in "nrq":
            data = read(d / f"a_1.scalce{e}")
            (d / f"bad_1.scalce{e}").write_bytes(data[:-cut] if e == ext else data)
        r = run_cli("-d", "--window", "256K", "-o", d / "x", d / "bad_1.scalcen", ok=False)
        assert r.returncode == 1 and b"(ERROR)" in r.stderr and b"truncated" in r.stderr, (ext, r.stderr[-300:])


# ---- 7: the C entry directly ----------------------------------------------------------------------------------------------
def test_stream_decompress_entry_with_small_pieces(tmp_path):
    from scalce_amd import host
    d = tmp_path
    make_inputs(d, 8000, 100, False, seed=71)
    run_cli("-c", "no", "-o", d / "a", d / "in_1.fq")
    r = run_cli("-d", "--window", "256K", "-o", d / "cli", d / "a_1.scalcen")
    want, nwin = read(d / "cli_1.fastq"), windows_line(r)[0]
    ctx = host.Context(0, patterns_bin=read(PBIN))
    for piece in (4093, 7):
        def reader(path, piece=piece):
            f = open(path, "rb")
            return lambda cap: f.read(min(cap, piece))
        got = []
        firsts = []

        def write(mate, first, nrec, text, offs):
            assert mate == 0 and offs is None and text.count(b"\n") == 4 * nrec
            firsts.append(first)
            got.append(text)
        st = host.stream_decompress(ctx, [[reader(d / f"a_1.scalce{e}") for e in "rnq"]], write, window_text_bytes=256 << 10)
        assert b"".join(got) == want, piece
        assert st.windows == nwin == len(got) and st.records[0] == 8000 and firsts == sorted(firsts) and firsts[0] == 0
        assert st.peak_device_bytes > 0 and st.window_text_bytes == 256 << 10
    with pytest.raises(host.ScalceError, match="truncated"):
        cut = read(d / "a_1.scalcer")[:-11]
        pos = [0]

        def short(cap):
            out = cut[pos[0]:pos[0] + cap]
            pos[0] += len(out)
            return out
        host.stream_decompress(ctx, [[short, reader(d / "a_1.scalcen", 1 << 20), reader(d / "a_1.scalceq", 1 << 20)]],
                               lambda *a: None, window_text_bytes=256 << 10)


# ---- 8: pipes ------------------------------------------------------------------------------------------------------------
def test_stdout_gets_the_windows(tmp_path):
    d = tmp_path
    make_inputs(d, 8000, 100, False, seed=73)
    run_cli("-c", "no", "-o", d / "a", d / "in_1.fq")
    run_cli("-d", "--window", "256K", "-o", d / "f", d / "a_1.scalcen")
    r = run_cli("-d", "--window", "256K", "-o", "-", d / "a_1.scalcen")
    assert r.stdout == read(d / "f_1.fastq") and windows_line(r)[0] >= 6


# ---- 9: the decoder's batches: carry at odd alignments, a batch cut short, archives that do not say how many records ------
def file_readers(d, stem, mates):
    def reader(path):
        f = open(path, "rb")
        return lambda cap: f.read(cap)
    return [[reader(d / f"{stem}_{m}.scalce{e}") for e in "rnq"] for m in range(1, mates + 1)]


def batches_of(d, stem, mates, window, **kw):
    """scalce_stream_decompress on the files the CLI read: (UnpackStats, the text per mate)"""
    from scalce_amd import host
    ctx = host.Context(0, patterns_bin=read(PBIN))
    got = {}
    st = host.stream_decompress(ctx, file_readers(d, stem, mates), lambda mate, first, n, text, offs: got.setdefault(mate, []).append(text),
                                mates=mates, window_text_bytes=window, **kw)
    return st, [b"".join(got[m]) for m in sorted(got)]


def test_carry_of_41_bytes_between_single_frame_batches(tmp_path):
    """--window 2M on reads of 101 bases: one frame per decoder batch, two frames, and 10 485 760 mod 101 = 41 symbols of the
    first carried in front of the second -- the decoder writes at Y + 41"""
    d = tmp_path
    n, L = 105000, 101
    assert n * L > 10485760 and 10485760 % L == 41
    make_inputs(d, n, L, False, seed=79)
    want = oracle_text(d, [], [], False)
    r = run_cli("-d", "--window", "2M", "-o", d / "back", d / "orc_1.scalcen")
    assert read(d / "back_1.fastq") == want[0]
    st, text = batches_of(d, "orc", 1, 2 << 20)
    assert text[0] == want[0]
    assert list(st.decode_batches) == [2, 0] and st.records[0] == n
    assert windows_line(r)[0] == st.windows >= -(-len(want[0]) // (2 << 20))


@pytest.mark.parametrize("n", [70000, 140000], ids=["70k_pairs", "140k_pairs"])
def test_interleaved_mates_each_with_a_carry_of_their_own(n, tmp_path):
    """-i, mates of 75 and 151 bases, --window 2M: one frame per batch in either mate.  Mate 2's second frame begins 18 symbols
    into a record (10 485 760 mod 151).  Mate 1 has a second frame, and its carry of 10 (10 485 760 mod 75), from 139 811 pairs
    on: at 70 000 pairs its stream is one frame and one batch beside mate 2's two; at 140 000 pairs mate 1 has two batches and
    mate 2 three, both write behind a carry, and their batches change at different windows.  (The larger case reads 31.6 M
    bases through the oracle twice: about 13 s, most of it on the CPU.  No smaller input gives mate 1 a second frame.)"""
    d = tmp_path
    assert 10485760 % 75 == 10 and 10485760 % 151 == 18
    synth.write_fastq(str(d / "in_1.fq"), n, 75, seed=89, n_frac=0.003, dup_frac=0.1, paired_suffix="/1")
    synth.write_fastq(str(d / "in_2.fq"), n, 151, seed=90, paired_suffix="/2")
    want = interleaved(*oracle_text(d, ["-r"], ["-r"], True))
    r = run_cli("-d", "-i", "--window", "2M", "-o", d / "back", d / "orc_1.scalcen")
    assert read(d / "back_1.fastq") == want
    st, text = batches_of(d, "orc", 2, 2 << 20, interleave=True)
    assert text == [want]
    assert list(st.decode_batches) == {70000: [1, 2], 140000: [2, 3]}[n] and list(st.records) == [n, n]
    assert windows_line(r)[0] == st.windows >= -(-len(want) // (2 << 20))


def test_batch_cut_short_by_frames_that_code_badly():
    """Three frames per batch (a window of 5.5 MB of text: 8 x 26 699 records x 100 > 2 x 10 485 760) and a stream that codes
    to three quarters of its symbols: the staging buffer takes two frames, not three, and the first batch is cut to them.
    The archive is built in memory -- made-up names, one root bucket, 3 x 10 485 760 + 50 000 symbols drawn uniformly from
    1..62 under a table of equal counts -- and coded by the oracle.  This is the smallest stream that reaches the cut."""
    from scalce_amd import host
    L, nsym, window = 100, 3 * R.FRAME + 50000, 5_500_000
    nrec = nsym // L
    rng = np.random.default_rng(97)
    sym = rng.integers(1, 63, size=nsym).astype(np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(nrec, L))]
    table = np.ones((6400, 80), dtype=np.uint32)
    table[:, 1:63] = 16
    coded = R.framed(table.reshape(-1), sym)
    sizes = [sz for _, sz in R.frames_of(coded, 4)]
    assert window // (2 * L + 6) * 8 * L > 2 * R.FRAME
    # three coded frames exceed 2 x 10 485 760 bytes and any two do not -- by more than the few KB the staging buffer has beside
    # that: whatever its exact size, it takes two of these frames and not three
    assert sum(4 + s for s in sizes[:3]) > 2 * R.FRAME + (1 << 20)
    assert all(8 + sizes[i] + sizes[j] < 2 * R.FRAME - (1 << 20) for i in range(4) for j in range(i))
    files = [R.read_stream_file(L, np.array([R.ROOT_CORE], dtype="<i4").tobytes() + np.array([nrec], dtype="<u8").tobytes() + R.pack_root_records(bases)),
             R.name_stream_file(library=b"cut"), R.quality_stream_file(33, table.reshape(-1), nsym, coded)]
    want = R.text_of_uniform(bases, sym[:nrec * L].reshape(nrec, L), b"cut", 0, 33)

    def reader(data):
        pos = [0]

        def rd(cap):
            out = data[pos[0]:pos[0] + cap]
            pos[0] += len(out)
            return out
        return rd
    got = []
    ctx = host.Context(0, patterns_bin=read(PBIN))
    st = host.stream_decompress(ctx, [[reader(f) for f in files]], lambda mate, first, n, text, offs: got.append(text), window_text_bytes=window)
    assert st.decode_batches[0] == 2 and st.records[0] == nrec
    text = b"".join(got)
    assert len(text) == len(want) and text == want
    print(f"cut batch: {st.windows} windows, decode {st.decode_s:.2f} s, total {st.total_s:.2f} s")


def greedy_windows(n, L, lib, window):
    """records per window when every window takes as many whole records as its text bound allows: a record of made-up names is
    "@<lib>.<index>" and 2 L + 6 more bytes of FASTQ, and no window holds more than window / (2 L + 6) records"""
    out, first = [], 0
    while first < n:
        k = text = 0
        while first + k < n and k < window // (2 * L + 6) and text + len(lib) + 1 + len(str(first + k)) + 2 * L + 6 <= window:
            text += len(lib) + 1 + len(str(first + k)) + 2 * L + 6
            k += 1
        out.append(k)
        first += k
    return out


@pytest.mark.parametrize("flag", ["-Q", "-A"])
@pytest.mark.parametrize("count", ["5R", "5R+1", "5_windows", "5_windows+1"])
def test_record_count_from_the_streams_under_small_windows(flag, count, tmp_path):
    """-Q -n lib and -A -n lib: neither a name stream nor a symbol count says how many records there are, the read stream
    (-Q) or the raw quality rows (-A) end the archive.  --window 64K; the archive holds a multiple of R = window / (2 L + 6)
    records, or ends with the last record that the fifth window's text takes -- and one record more."""
    d = tmp_path
    L, window = 100, 64 << 10
    R_ = window // (2 * L + 6)
    five = sum(greedy_windows(10 * R_, L, "lib", window)[:5])
    n = {"5R": 5 * R_, "5R+1": 5 * R_ + 1, "5_windows": five, "5_windows+1": five + 1}[count]
    make_inputs(d, n, L, False, seed=101)
    cflags = ["-n", "lib"] + (["-A"] if flag == "-A" else [])
    want = oracle_text(d, cflags, ["-n", "lib"], False)[0]
    if flag == "-Q":
        want = two_line(want)
        run_cli("-Q", "-n", "lib", "-c", "no", "-o", d / "hip", d / "in_1.fq")
    stem = "hip" if flag == "-Q" else "orc"
    r = run_cli("-d", "-n", "lib", *(["-Q"] if flag == "-Q" else []), "--window", "64K", "-o", d / "back", d / f"{stem}_1.scalcen")
    assert read(d / "back_1.fastq") == want
    assert want.count(b"\n") == n * (2 if flag == "-Q" else 4) and b"@lib.%d\n" % (n - 1) in want
    nwin = windows_line(r)[0]
    assert nwin == len(greedy_windows(n, L, "lib", window))
    if count.startswith("5_windows"):
        assert nwin == (6 if count.endswith("+1") else 5)
