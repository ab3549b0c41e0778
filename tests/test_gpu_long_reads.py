"""-m gpu: every stage at read lengths of 301 to 2498 bases, the nine tenths of the supported range behind the other tests' 301.

The inputs are those of tests/long_reads.py; tests/test_long_reads_cpu.py holds them to what they claim with the oracle alone.
Here the device is compared with the oracle stage by stage (gpu_util.check_against_oracle: tokens, permutation, q', trigram
counters, scaled table, reordered quality stream, coded bytes), then file by file through the command line, both directions:
two-byte `end` values up to 2498, twenty probe segments of the anchor walk, 157 words of the k-mer walk, ties of hundreds of
candidates, 625 key digits with runs on both sides of the small sort's 32, records of 5 KB through the direct ingest kernel,
the varlen pad and strip, exception positions with the 2048 bit set, windows and ranges smaller than one record."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bigtable as B
import decode_ref as DR
import exception_ref as ER
import filecases as F
import gpu_util as G
import ingest_ref as IR
import long_reads as LR
import oraclelib as O
import varlen_util as V
from scalce_amd import host

pytestmark = pytest.mark.gpu
LMAX = LR.MAX_LENGTH
MAGIC = b"scalce22"


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def scalce(*args, ok=True, env=None, table=None):
    table = ["--patterns-bin", F.PBIN] if table is None else ["-P", str(table)]
    r = subprocess.run([F.SCALCE, *map(str, args), *table], capture_output=True, timeout=600,
                       env=None if env is None else dict(os.environ, **env))
    if ok is not None:
        assert (r.returncode == 0) == ok, (args, r.returncode, r.stderr[-1500:])
    return r


def read(p):
    return open(p, "rb").read()


def write(p, data):
    with open(p, "wb") as f:
        f.write(data)
    return p


def same_archive(d, a, b, mates=(1,), exts="nrq"):
    for m in mates:
        for ext in exts:
            x, y = F.content(os.path.join(str(d), "%s_%d.scalce%s" % (a, m, ext))), F.content(os.path.join(str(d), "%s_%d.scalce%s" % (b, m, ext)))
            assert x == y, ".scalce%s of mate %d: %s holds %d bytes, %s %d" % (ext, m, a, len(x), b, len(y))


def direct_ingest_and_scanned_rows(b):
    assert b.ingest_plan(0)[0] == 3, "reads above 160 bases go through the direct indexed kernel"
    assert b.quality_plan(0)[0] == 2, "the statistics come from the scan of the q' rows"


# ---- stage parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LR.LONG)
def test_stage_parity_per_length(L, ctx, oracle_trie):
    bases, quals = LR.genome(257, L)
    b, ref, st = G.check_against_oracle(ctx, oracle_trie, bases, quals, label="genome L=%d" % L)
    direct_ingest_and_scanned_rows(b)
    assert (ref["pat"] >= 0).sum() > 200 and ref["end"].max() > min(L, 300) - 50


def test_stage_parity_more_than_one_tokenizer_workgroup(ctx, oracle_trie):
    bases, quals = LR.genome(1025, LMAX)
    b, ref, st = G.check_against_oracle(ctx, oracle_trie, bases, quals, label="genome 1025 x 2498")
    direct_ingest_and_scanned_rows(b)
    assert ref["end"].max() > 2400 and st["tie_reads"] > 0


# ---- crafted cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1000, LMAX])
def test_ends(L, ctx, oracle_trie):
    bases, quals, targets, coreless = LR.ends(L)
    b, ref, st = G.check_against_oracle(ctx, oracle_trie, bases, quals, label="ends L=%d" % L)
    assert sorted(ref["end"][ref["pat"] >= 0]) == targets and (ref["pat"] < 0).sum() == coreless
    # the read stream decoded on the host: each record's two metadata bytes spell its `end`, its bases are the read's
    payload = b.output(host.OUT_READS, 0).tobytes()
    reads, cores, ends = DR.unpack_records(payload, L, lambda cid: oracle_trie.pattern(cid))
    perm = ref["perm"]
    assert ends == ref["end"][perm].tolist()
    assert reads == [bases[int(r)].tobytes() for r in perm]
    assert [c[0] for c in cores][-1] == DR.ROOT_CORE and sum(c[2] for c in cores) == len(bases)
    assert DR.sz_meta(L) == 2 and max(ends) == L and any(e >> 8 > 1 for e in ends)


@pytest.mark.parametrize("L", [1000, LMAX])
def test_many_candidates(L, ctx, oracle_trie):
    bases, quals = LR.many_candidates(L)
    b, ref, st = G.check_against_oracle(ctx, oracle_trie, bases, quals, label="many_candidates L=%d" % L)
    assert st["tie_reads"] == len(bases), st
    assert (ref["pat"] >= 0).all() and (ref["end"] > 12).any()


@pytest.mark.parametrize("L", [1000, LMAX])
def test_prefix_runs(L, ctx, oracle_trie):
    bases, quals, group, where = LR.prefix_runs(L)
    b, ref, st = G.check_against_oracle(ctx, oracle_trie, bases, quals, label="prefix_runs L=%d" % L)
    members, fallback, starts, lens = G.order_expectation(bases, ref["pat"], ref["end"], ref["perm"])
    assert sorted(lens.tolist()) == sorted(LR.RUN_SIZES) and fallback
    assert st["order_run_members"] == members == sum(LR.RUN_SIZES), st
    assert st["order_radix_fallback"] != 0, "the run of 40 takes the radix passes"


@pytest.mark.parametrize("walk", ["kmer", "anchor"])
def test_homopolymer_table(walk):
    text = LR.homopolymer_table(walk)
    c, trie = host.Context(0, patterns_text=text), O.Trie(text=text)
    assert c.walk == (("kmer", 0) if walk == "kmer" else ("anchor", 8))
    bases, quals, kinds = LR.homopolymer_reads(LMAX)
    b, ref, st = G.check_against_oracle(c, trie, bases, quals, label="homopolymer " + walk)
    got = [(trie.pattern(int(p)).decode(), int(e)) for p, e in zip(ref["pat"], ref["end"])]
    assert got == LR.homopolymer_expectation(kinds, LMAX)
    assert st["tie_reads"] >= sum(len(k) == 2 for k in kinds), st


# ---- both tokenizer walks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["shipped", "short_t7", "anchor_k8", "single"])
def test_both_tokenizer_walks_at_the_limit(shape, ctx, oracle_trie):
    """the stage-parity input under a table of each walk kind, and reads that carry the table's own cores at the corners of the
    walks (bigtable.corner_reads): across each of the twenty 128-position segments, at every offset of a 16-base word"""
    if shape == "shipped":
        c, trie, cores, walk = ctx, oracle_trie, [x.decode() for _, x in LR.shipped_table()[2]], ("kmer", 0)
    else:
        t = B.shape(shape)
        c = host.Context(0, patterns_text=t.blob) if t.text else host.Context(0, patterns_bin=t.blob)
        trie = O.Trie(text=t.blob) if t.text else O.Trie(blob=t.blob)
        cores, walk = t.cores, t.walk
    assert c.walk == walk
    gb, gq = LR.genome(129, LMAX)
    cb = B.corner_reads(cores, LMAX, 128, seed=LMAX)
    bases = np.concatenate([gb, cb])[np.random.default_rng(3).permutation(257)]
    quals = np.concatenate([gq, gq[:128]])
    b, ref, st = G.check_against_oracle(c, trie, bases, quals, label="walk of " + shape)
    assert (ref["pat"] >= 0).sum() > 128 and ref["end"].max() > 2400


# ---- pairs ----------------------------------------------------------------------------------------------------------------
def has_coreless_read(scalcer, L, lens):
    pos, meta = 16, (2 if L > 255 else 1)
    while pos + 12 <= len(scalcer):
        core, cnt = struct.unpack_from("<iq", scalcer, pos)
        if core == host.ROOT_CORE:
            return True
        pos += 12 + cnt * ((L - int(lens[core]) + 3) // 4 + meta)
    return False


PAIRS = [(2498, 36), (36, 2498), (1000, 1000), (255, 256), (256, 255)]


@pytest.fixture(scope="module")
def pair_case(tmp_path_factory):
    """the inputs of a pair of read lengths and the oracle's archive and restored text of them, made once"""
    made = {}

    def get(L1, L2):
        if (L1, L2) not in made:
            d = tmp_path_factory.mktemp("pairs_%d_%d" % (L1, L2))
            n = 300
            b1, q1 = LR.genome(n, L1, seed=LR.seed_of("pairs/1", L1, L2))
            b2, q2 = LR.genome(n, L2, seed=LR.seed_of("pairs/2", L1, L2))
            b1[7] = LR.row(LR.filler_for(L1), L1)     # a coreless read: without one the reference's decoder spoils mate 2 (test_gpu_fuzz.py)
            t1, t2 = LR.fastq(b1, q1, "p.", "/1"), LR.fastq(b2, q2, "p.", "/2")
            write(d / "in_1.fq", t1)
            write(d / "in_2.fq", t2)
            write(d / "il.fq", b"".join(x + y for x, y in zip(V.records_of(t1), V.records_of(t2))))
            O.orc_cli("compress", F.PBIN, d / "in_1.fq", d / "orc", "-r")
            O.orc_cli("decompress", F.PBIN, d / "orc_1.scalcen", d / "oback", "-r")
            made[L1, L2] = d
        return made[L1, L2]
    return get


@pytest.mark.parametrize("L1,L2", PAIRS)
def test_pairs_in_two_files(L1, L2, pair_case, oracle_trie):
    d = pair_case(L1, L2)
    scalce("-r", "-c", "no", "-o", d / "hip", d / "in_1.fq")
    same_archive(d, "hip", "orc", (1, 2))
    assert has_coreless_read(F.content(str(d / "hip_1.scalcer")), L1, oracle_trie.pattern_lens())
    scalce("-d", "-r", "-o", d / "back", d / "hip_1.scalcen")
    for m in (1, 2):
        assert read(d / ("back_%d.fastq" % m)) == read(d / ("oback_%d.fastq" % m)), "mate %d" % m


@pytest.mark.parametrize("L1,L2", PAIRS)
def test_pairs_interleaved(L1, L2, pair_case):
    d = pair_case(L1, L2)
    scalce("-i", "-c", "no", "-o", d / "il", d / "il.fq")
    same_archive(d, "il", "orc", (1, 2))
    scalce("-d", "-i", "-o", d / "ilback", d / "il_1.scalcen")
    want = [V.records_of(read(d / ("oback_%d.fastq" % m))) for m in (1, 2)]
    assert read(d / "ilback_1.fastq") == b"".join(x + y for x, y in zip(*want))


# ---- the command line at 400 reads of 2498 bases --------------------------------------------------------------------------
N_CLI = 400


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("long_cli")
    bases, quals = LR.genome(N_CLI, LMAX)
    text = LR.fastq(bases, quals)
    write(d / "in_1.fq", text)
    O.orc_cli("compress", F.PBIN, d / "in_1.fq", d / "orc")
    O.orc_cli("decompress", F.PBIN, d / "orc_1.scalcen", d / "oback")
    scalce("-c", "no", "-o", d / "hip", d / "in_1.fq")
    return dict(d=d, bases=bases, quals=quals, text=text, oback=read(d / "oback_1.fastq"))


CLI_FLAGS = {"plain": [], "A": ["-A"], "nlib": ["-n", "lib"], "p30": ["-p", "30"], "B1M": ["-B", "1M"], "gz": ["-c", "gz"]}


@pytest.mark.parametrize("name", list(CLI_FLAGS))
def test_cli_parity(name, cli_input, tmp_path):
    d, flags = cli_input["d"], CLI_FLAGS[name]
    oflags = [str(1 << 20) if f == "1M" else f for f in flags]
    r = scalce(*flags, *([] if "-c" in flags else ["-c", "no"]), "-o", tmp_path / "hip", d / "in_1.fq")
    O.orc_cli("compress", F.PBIN, d / "in_1.fq", tmp_path / "orc", *oflags)
    same_archive(tmp_path, "hip", "orc")
    if name == "B1M":    # the smallest -B the command line takes, as the reference's
        line = next(ln for ln in r.stderr.decode().splitlines() if "Spill chunks" in ln)
        assert int(line.split("Spill chunks:")[1].split(",")[0]) == expected_chunks(cli_input, 1 << 20) == 2, line
    dflags = ["-n", "lib"] if name == "nlib" else []
    scalce("-d", *dflags, "-o", tmp_path / "back", tmp_path / "hip_1.scalcen")
    O.orc_cli("decompress", F.PBIN, tmp_path / "orc_1.scalcen", tmp_path / "oback", *dflags)
    O.orc_cli("decompress", F.PBIN, tmp_path / "hip_1.scalcen", tmp_path / "ohback", *dflags)   # the oracle reads the HIP archive
    want = read(tmp_path / "oback_1.fastq")
    assert read(tmp_path / "back_1.fastq") == want and read(tmp_path / "ohback_1.fastq") == want
    assert want.count(b"\n") == 4 * N_CLI


def expected_chunks(cli_input, limit):
    """the -B rule (gpu_util.chunks_by_rule) on the oracle's tokens: a record of 2498 bases adds about 3.2 KB to its chunk"""
    trie = LR.shipped_table()[1]
    pat, _ = trie.tokenize(cli_input["bases"])
    name_lens = [len("s.%d" % i) for i in range(N_CLI)]
    return G.chunks_by_rule(G.record_sizes(pat, trie.pattern_lens(), name_lens, LMAX), limit)[1]


def test_spill_chunks_of_twenty_records(cli_input, ctx, tmp_path):
    """-B 64K: the command line takes M and G alone, as the reference's does, so the chunk size goes in through the C ABI
    (bucket_set_size) and the streams are written out as test_gpu_parity.py does; the oracle's CLI takes the bytes"""
    from scalce_amd import format as fmt
    d = cli_input["d"]
    off, vals, Ls = fmt.sample_qmap(cli_input["text"])
    assert Ls == LMAX
    b = G.hip_compress(ctx, cli_input["text"], LMAX, qmap=[(off, vals), (off, vals)], bucket_set_size=65536)
    assert b.stats()["chunks"] == expected_chunks(cli_input, 65536) == 20, b.stats()     # about twenty records each
    fmt.write_archive(str(tmp_path / "hip"), b, off, library="lib")
    O.orc_cli("compress", F.PBIN, d / "in_1.fq", tmp_path / "orc", "-B", 65536)
    same_archive(tmp_path, "hip", "orc")
    scalce("-d", "-o", tmp_path / "back", tmp_path / "hip_1.scalcen")
    O.orc_cli("decompress", F.PBIN, tmp_path / "orc_1.scalcen", tmp_path / "oback")
    assert read(tmp_path / "back_1.fastq") == read(tmp_path / "oback_1.fastq")


@pytest.mark.parametrize("mode", ["-Q", "-f"])
def test_cli_without_qualities(mode, cli_input, tmp_path):
    """the read and name streams are the oracle's of the run with qualities, the quality file is its header alone, and -d writes
    the two-line records in the archive's order"""
    import test_gpu_no_qualities as NQ
    d = cli_input["d"]
    src = write(tmp_path / "x_1.fq", NQ.to_fasta(cli_input["text"]) if mode == "-f" else cli_input["text"])
    scalce(mode, "-c", "no", "-o", tmp_path / "nq", src)
    for ext in "rn":
        assert read(tmp_path / ("nq_1.scalce" + ext)) == read(d / ("orc_1.scalce" + ext)), ext
    assert read(tmp_path / "nq_1.scalceq") == MAGIC + struct.pack("<q", 64 if mode == "-f" else 33)
    scalce("-d", mode, "-o", tmp_path / "back", tmp_path / "nq_1.scalcen")
    assert read(tmp_path / "back_1.fastq") == NQ.expected_two_line(cli_input["oback"], cli_input["text"])


@pytest.mark.parametrize("piece", [4096, 8192, 30000])
def test_cli_pieces_smaller_than_a_record(piece, cli_input, tmp_path):
    """SCALCE_PIECE_BYTES of 4096 is less than one record of 5 KB: the streaming host raises a piece to hold one record at its
    bound, so the run goes through and writes the one-piece archive"""
    d = cli_input["d"]
    r = scalce("-c", "no", "-o", tmp_path / "hip", d / "in_1.fq", env=dict(SCALCE_PIECE_BYTES=str(piece)))
    assert b"pieces streamed" in r.stderr
    for ext in "nrq":
        assert read(tmp_path / ("hip_1.scalce" + ext)) == read(d / ("hip_1.scalce" + ext)), ext
    same_archive(d, "hip", "orc")


# ---- windows and ranges ---------------------------------------------------------------------------------------------------
def windows_of(r):
    return int(next(ln for ln in r.stderr.decode().splitlines() if "Windows:" in ln).split("Windows:")[1].split()[0])


@pytest.mark.parametrize("window,count", [(1, N_CLI), (3000, N_CLI), ("three", -(-N_CLI // 3))], ids=["one_byte", "below_one_record", "three_records"])
def test_windows_smaller_than_a_record(window, count, cli_input, tmp_path):
    d = cli_input["d"]
    rec = 2 * LMAX + 6 + 255 + 32          # a record's text at its bound (the window loop's)
    w = 3 * rec if window == "three" else window
    r = scalce("-d", "--window", w, "-o", tmp_path / "back", d / "hip_1.scalcen")
    assert read(tmp_path / "back_1.fastq") == cli_input["oback"]
    assert windows_of(r) == count


SLICES = ((0, 1), (1, 136), (137, 100), (237, N_CLI - 238), (N_CLI - 1, 5))


@pytest.mark.parametrize("first,cnt", [(0, 1), (1, 1), (N_CLI - 1, 1), (137, 100)])
def test_record_range_under_a_window_below_one_record(first, cnt, cli_input, tmp_path):
    """(every record but the first begins inside the archive's one coder frame)"""
    recs = V.records_of(cli_input["oback"])
    scalce("-d", "--records", "%d:%d" % (first, cnt), "--window", 3000, "-o", tmp_path / "r", cli_input["d"] / "hip_1.scalcen")
    assert read(tmp_path / "r_1.fastq") == b"".join(recs[first:first + cnt])


@pytest.mark.parametrize("k", range(len(SLICES)))
def test_record_slices_concatenate_to_the_whole(k, cli_input, tmp_path):
    recs = V.records_of(cli_input["oback"])
    a, cnt = SLICES[k]
    assert sum(min(c, N_CLI - s) for s, c in SLICES) == N_CLI and all(SLICES[i][0] + SLICES[i][1] == SLICES[i + 1][0] for i in range(len(SLICES) - 1))
    scalce("-d", "--records", "%d:%d" % (a, cnt), "-o", tmp_path / "s", cli_input["d"] / "hip_1.scalcen")
    assert read(tmp_path / "s_1.fastq") == b"".join(recs[a:a + cnt])


# ---- variable length ------------------------------------------------------------------------------------------------------
def test_variable_length_batch(ctx, oracle_trie):
    import test_gpu_varlen as TV
    L = LMAX
    lens = LR.varlen_lengths(L)
    var, pad = TV.check_identity(ctx, L, lens, 71)         # the padded twin's outputs, and OUT_LENGTHS in output order
    want = IR.ingest(pad, L)
    assert want.error is None and want.nrec == len(lens)
    b = G.hip_compress(ctx, var, L, variable_length=True)
    direct_ingest_and_scanned_rows(b)
    assert (b.output(host.OUT_QINPUT, 0).reshape(len(lens), L) == want.qp[0]).all(), "the padded q' rows"
    pat, end = oracle_trie.tokenize(want.bases[0])
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    assert (tok[:, 0] == pat).all() and (tok[:, 1] == end).all(), "tokens of the padded rows"
    perm = oracle_trie.order(want.bases[0], pat, end)
    assert (b.output(host.OUT_PERM, 0, np.uint32) == perm).all()
    got = b.output(host.OUT_LENGTHS, 0, np.uint16)
    assert (got == (L - lens)[perm]).all() and got.max() == L and (got > 255).any()


def test_variable_length_cli(tmp_path):
    L = LMAX
    lens = LR.varlen_lengths(L)
    var, pad, names = V.texts(L, lens, 72)
    write(tmp_path / "var_1.fq", var)
    write(tmp_path / "pad_1.fq", pad)
    scalce("--max-length", L, "-c", "no", "-o", tmp_path / "ours", tmp_path / "var_1.fq")
    O.orc_cli("compress", F.PBIN, tmp_path / "pad_1.fq", tmp_path / "orc")
    same_archive(tmp_path, "ours", "orc")
    if os.path.exists(F.REF_FULL):     # the reference's own archive of the padded text, as test_gpu_varlen_cli.py states it
        r = subprocess.run([F.REF_FULL, "compress", F.PBIN, str(tmp_path / "pad_1.fq"), str(tmp_path / "ref"), "-T", "1", "-t",
                            str(tmp_path / "tmp_ref")], capture_output=True)
        assert r.returncode == 0, r.stderr[-1500:]
        same_archive(tmp_path, "ours", "ref")
    stored_L, entries = host_lengths(read(tmp_path / "ours_1.scalcel"))
    assert stored_L == L and sorted(entries) == sorted(L - lens)
    O.orc_cli("decompress", F.PBIN, tmp_path / "ours_1.scalcen", tmp_path / "oback")
    want = V.cut_to_lengths(read(tmp_path / "oback_1.fastq"), dict(zip(names, lens)))
    for k, w in enumerate(([], ["--window", 3000])):
        scalce("-d", *w, "-o", tmp_path / ("rt%d" % k), tmp_path / "ours_1.scalcen")
        assert read(tmp_path / ("rt%d_1.fastq" % k)) == want
    assert len(want) < len(pad) and sorted(V.records_of(want)) != sorted(V.records_of(pad))


def host_lengths(data):
    from scalce_amd import format as FMT
    return FMT.unpack_lengths(data)


def test_reads_longer_than_the_limit_are_errors_that_leave_no_archive(tmp_path):
    bases, quals = LR.genome(20, LMAX + 1, n_frac=0)
    src = write(tmp_path / "in_1.fq", LR.fastq(bases, quals))
    r = scalce("-c", "no", "-o", tmp_path / "a", src, ok=False)
    assert r.returncode == 1 and b"2498" in r.stderr, r.stderr[-400:]
    r = scalce("--max-length", LMAX + 1, "-c", "no", "-o", tmp_path / "b", src, ok=False)
    assert r.returncode == 1 and b"--max-length" in r.stderr and b"2498" in r.stderr, r.stderr[-400:]
    r = scalce("--variable-length", "-c", "no", "-o", tmp_path / "c", src, ok=False)
    assert r.returncode == 1, r.stderr[-400:]
    assert not [f for f in os.listdir(tmp_path) if ".scalce" in f]


# ---- kept bases, comments, order ------------------------------------------------------------------------------------------
def test_exceptions_batch(ctx):
    import test_gpu_exceptions as TE
    bases, quals, at = LR.exception_patterns(LMAX)
    bk = TE.check_against_plain(ctx, bases, quals)    # exception_ref's entries in OUT_PERM order, exceptions_info, every other output
    e = bk.output(host.OUT_EXCEPTIONS, 0, np.uint64)
    pos = (e >> np.uint64(16)) & np.uint64(0xFFF)
    rec = (e >> np.uint64(28)).astype(np.int64)
    perm = bk.output(host.OUT_PERM, 0, np.uint32)
    assert sorted(pos[perm[rec] == 0].tolist()) == at and (pos >= 2048).any()
    assert (perm[rec] == 1).sum() == LMAX and (perm[rec] == 2).sum() == LMAX          # 2498 entries in one record's count
    x, rows = bk.exceptions_info(0)
    assert x == len(e) == int(ER.exception_mask(bases, quals).sum()) and rows > 30


def test_exception_apply_pass_on_a_window_of_long_records(ctx):
    import test_gpu_exceptions as TE
    n, L, first = 5, LMAX, 1000
    bases, quals = LR.genome(n, L, seed=LR.seed_of("apply"), n_frac=0)
    recs = [b"@" + nm + b"\n" + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n"
            for i, nm in enumerate((b"a", b"b" * 255, b"lib.1002", b"", b"e"))]
    picks = sorted({(r, p) for r in range(n) for p in (0, 2047, 2048, L - 1)} | {(3, p) for p in range(L)})
    ents = [host.exception_entry(first + r, p, int(b"acgtn"[(r + p) % 5]), 35 + (r + p) % 40) for r, p in picks]
    got, bad = TE.apply_on_device(ctx, recs, L, True, first, ents)
    assert bad == 0 and got == b"".join(ER.apply_text(recs, ents, L, True, first=first)) and got != b"".join(recs)
    got, bad = TE.apply_on_device(ctx, recs, L, True, first, [host.exception_entry(first, L, ord("n"), 40)])
    assert bad == 1 and got == b"".join(recs)


@pytest.mark.parametrize("case", ["fixed", "varlen"])
def test_keep_options_return_the_input(case, tmp_path):
    L = LMAX
    bases, quals, _ = LR.exception_patterns(L)
    lens = None
    if case == "varlen":
        lens = np.resize(LR.varlen_lengths(L), len(bases))
    text = LR.fastq(bases, quals, prefix="r.", lens=lens, comments=True)
    src = write(tmp_path / "in_1.fq", text)
    flags = ["--max-length", L] if case == "varlen" else []
    scalce(*flags, "--keep-order", "--keep-comments", "--keep-bases", "-p", "0", "-c", "no", "-o", tmp_path / "a", src)
    for k, w in enumerate(([], ["--window", 1])):
        scalce("-d", *w, "-o", tmp_path / ("back%d" % k), tmp_path / "a_1.scalcen")
        assert read(tmp_path / ("back%d_1.fastq" % k)) == text, "window %s" % w
    Lx, n, ents = host.unpack_exceptions(F.content(str(tmp_path / "a_1.scalcex")))
    assert (Lx, n) == (L, len(bases)) and (((ents >> np.uint64(16)) & np.uint64(0xFFF)) >= 2048).any()
