"""-m gpu: the tie-break at its edges -- prior counts, window boundaries, candidate lists, the sequential way out.

Every case tokenizes a small batch (ingest + scalce_batch_tokenize, nothing behind it) and compares OUT_TOKENS row by row
and OUT_BUCKET_COUNTS bucket by bucket with tests/tie_ref.py's sequential rule, which tests/test_tie_ref_cpu.py holds against
the oracle and whose inputs that file shows to be what the cases need.  The path is chosen with SCALCE_TIE_WINDOW and
SCALCE_TIE_MAX_SWEEPS and asserted through Batch.tie_plan() and stats()["tie_fallback"]: a case whose hook did not select
the path it is named after fails."""
import numpy as np
import pytest

import tie_ref as T
from gpu_util import device_bytes
from scalce_amd import host

pytestmark = pytest.mark.gpu
DEFAULT_WINDOW = 196608
WINDOW_CLAMP = 1 << 30
FUSED, TWO, GLOBAL = 1, 2, 3               # tie_plan()["path"]
SEQ_LDS, SEQ_LDS_RAISED, SEQ_GLOBAL = 1, 2, 3   # tie_plan()["sequential"]
# name -> (environment, path, tie reads per window asked for, ends in tie_sequential_k)
PATHS = {
    "default": ({}, FUSED, DEFAULT_WINDOW, False),
    "fused": ({"SCALCE_TIE_WINDOW": "100"}, FUSED, 100, False),
    "two_launches": ({"SCALCE_TIE_WINDOW": "100:two_launches"}, TWO, 100, False),
    "global": ({"SCALCE_TIE_WINDOW": "0"}, GLOBAL, 0, False),
    # a window is seen settled by a sweep that moves nothing: with one sweep allowed per window none ever is
    "sequential": ({"SCALCE_TIE_MAX_SWEEPS": "1"}, FUSED, DEFAULT_WINDOW, True),
    "sequential_two": ({"SCALCE_TIE_WINDOW": "100:two_launches", "SCALCE_TIE_MAX_SWEEPS": "1"}, TWO, 100, True),
    # the global sweeps go out four at a time: an input that needs more than four (test_tie_ref_cpu.py) has not settled then
    "sequential_global": ({"SCALCE_TIE_WINDOW": "0", "SCALCE_TIE_MAX_SWEEPS": "1"}, GLOBAL, 0, True),
}
_CTX, _TEXT, _WANT = {}, {}, {}


def use_path(monkeypatch, env):
    for k in ("SCALCE_TIE_WINDOW", "SCALCE_TIE_MAX_SWEEPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def context(t):
    """(device context, pattern of every bucket with T.ROOT for the root bucket), once per table"""
    if t.name not in _CTX:
        ctx = host.Context(0, patterns_text=t.blob) if t.text else host.Context(0, patterns_bin=t.blob)
        assert ctx.walk == t.walk, f"{t.name}: the table selects {ctx.walk}, the case is written for {t.walk}"
        bp = [T.ROOT if p == host.ROOT_CORE else int(p) for p in ctx.bucket_patterns()]
        assert bp[-1] == T.ROOT and sorted(bp[:-1]) == list(range(len(t.cores))) and len(bp) == ctx.n_buckets + 1
        _CTX[t.name] = (ctx, bp)
    return _CTX[t.name]


def sequential_counters(nb1):
    """where tie_sequential_k keeps nb1 counters of four bytes"""
    return SEQ_LDS if 4 * nb1 <= 48 * 1024 else SEQ_LDS_RAISED if 4 * nb1 <= 100 * 1024 else SEQ_GLOBAL


def device_prior(bp, prior):
    """a prior (pattern -> reads) as the device's u64 per bucket; None stays None (no prior at all)"""
    import torch
    if prior is None:
        return None
    a = np.array([prior.get(p, 0) for p in bp], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def expected(name, prior_name, prior):
    """tie_ref.settle of an input under a prior, once per module: (tokens as an int32 array, counts)"""
    if (name, prior_name) not in _WANT:
        toks, own = T.settle(T.input_candidates(name)[2], None, prior)
        _WANT[name, prior_name] = (np.array(toks, dtype=np.int32).reshape(-1, 2), own)
    return _WANT[name, prior_name]


def text_of(name):
    if name not in _TEXT:
        _TEXT[name] = T.fastq(T.inputs(name)[1])
    return _TEXT[name]


def tokenize(name, prior=None):
    """the input as one piece: ingest, tokenize under the prior -> (batch, buckets' patterns)"""
    t, reads = T.inputs(name)
    ctx, bp = context(t)
    fq = text_of(name)
    d = device_bytes(fq)
    b = host.Batch(ctx, len(reads[0]), len(reads) + 8, len(fq) + 64)
    dp = device_prior(bp, prior)
    b.ingest(0, d.data_ptr(), len(fq))
    b.tokenize(dp.data_ptr() if dp is not None else None)
    b._keep = (d, dp)
    assert b.n_reads == len(reads)
    return b, bp


def check_tokens(b, bp, want_tok, want_counts, what):
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    assert tok.shape == want_tok.shape, f"{what}: {tok.shape[0]} rows of tokens, {want_tok.shape[0]} reads"
    bad = np.flatnonzero((tok != want_tok).any(axis=1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(tok)} reads differ, first {bad[:4]}: device {tok[bad[:4]].tolist()} "
                           f"reference {want_tok[bad[:4]].tolist()} ({b.stats()}, {b.tie_plan()})")
    counts = b.output(host.OUT_BUCKET_COUNTS, 0, np.uint64)
    want = np.array([want_counts.get(p, 0) for p in bp], dtype=np.uint64)
    badc = np.flatnonzero(counts != want)
    assert len(badc) == 0, f"{what}: {len(badc)} bucket counts differ, first {badc[:4]}: {counts[badc[:4]]} for {want[badc[:4]]}"


def check_plan(b, ntie, path, window, fallback, nb1, what):
    """the path the case is written for: tie_plan() and stats() of the last tokenize"""
    plan, st = b.tie_plan(), b.stats()
    assert st["tie_reads"] == ntie, f"{what}: {st['tie_reads']} tie reads, the reference finds {ntie}"
    if ntie == 0:
        assert plan == dict(path=0, window=0, windows=0, sequential=0) and st["tie_fallback"] == 0, f"{what}: {plan} {st}"
        return
    w = min(window, WINDOW_CLAMP)
    want = dict(path=path, window=w, windows=-(-ntie // w) if w else 0, sequential=sequential_counters(nb1) if fallback else 0)
    assert plan == want, f"{what}: took {plan}, written for {want} ({st})"
    assert st["tie_fallback"] == int(fallback), f"{what}: {st}"
    assert st["jacobi_iters"] >= 1


def run_case(monkeypatch, name, path_name, prior_name="none", prior=None, path=None):
    env, kind, window, fallback = path if path is not None else PATHS[path_name]
    use_path(monkeypatch, env)
    t, reads, cands = T.input_candidates(name)
    b, bp = tokenize(name, prior)
    what = f"{name} {path_name} prior {prior_name}"
    check_plan(b, len(T.tie_rows(cands)), kind, window, fallback, len(bp), what)
    check_tokens(b, bp, *expected(name, prior_name, prior), what)
    return b


# ---- priors ---------------------------------------------------------------------------------------------------------------
PRIOR_NAMES = ("none", "zero", "prefix", "equal", "last_ahead", "above_2_33", "root_only", "high_bits")


@pytest.mark.parametrize("prior_name", PRIOR_NAMES)
@pytest.mark.parametrize("path_name", ["default", "fused", "two_launches", "global", "sequential"])
def test_priors(path_name, prior_name, monkeypatch):
    """no prior, all zero, the counts of the 2048 reads in front, the same on every bucket, ranks that put a read's last
    candidate ahead, 2^33 + 5 or 6 on every bucket, the root bucket alone, counts whose upper and lower 32 bits rank the
    buckets in opposite orders -- through every path"""
    prior = T.priors_under_test()[prior_name][0]
    assert (prior is None) == (prior_name == "none")
    run_case(monkeypatch, "priors", path_name, prior_name, prior)


@pytest.mark.parametrize("prior_name", ["prefix", "above_2_33", "high_bits"])
@pytest.mark.parametrize("path_name", ["fused", "two_launches", "global", "sequential", "sequential_global"])
def test_pieces_under_a_prior(path_name, prior_name, monkeypatch):
    """two pieces appended without tokenizing, each then tokenized under the prior: the second one is settled against the
    prior and the first one's reads, so both together are the sequential rule over all rows from that prior"""
    env, kind, window, fallback = PATHS[path_name]
    use_path(monkeypatch, env)
    t, reads, cands = T.input_candidates("priors")
    ctx, bp = context(t)
    prior = T.priors_under_test()[prior_name][0]
    dp = device_prior(bp, prior)
    cut = T.PIECE_CUT
    want_tok, want_counts = expected("priors", prior_name, prior)
    first_counts = T.settle(cands[:cut], None, prior)[1]
    b = host.Batch(ctx, len(reads[0]), len(reads) + 8, len(text_of("priors")) + 64)
    keep = []
    for k, (lo, hi) in enumerate(((0, cut), (cut, len(reads)))):
        fq = T.fastq(reads[lo:hi])
        d = device_bytes(fq)
        keep.append(d)
        used = b.append(d.data_ptr(), len(fq), final=k == 1, flags=host.APPEND_NO_TOKENIZE | host.APPEND_NO_QUALITY)
        assert used[0] == len(fq) and b.n_reads == hi
        b.tokenize(dp.data_ptr())
        what = f"piece {k} {path_name} prior {prior_name}"
        check_plan(b, len(T.tie_rows(cands[lo:hi])), kind, window, fallback, len(bp), what)
        check_tokens(b, bp, want_tok[:hi], first_counts if k == 0 else want_counts, what)


# ---- window edges ---------------------------------------------------------------------------------------------------------
def windows_of(ntie):
    ws = [1, 2, 31, 32, 33, 63, 64, 65, ntie - 1, ntie, ntie + 1, 1 << 31]
    return ws + ([ntie // 2] if ntie % 2 == 0 else [])


N_TWO, N_MIXED = 200, 227   # tie reads of the inputs "two" and "mixed" (asserted against the reference in every case)


@pytest.mark.parametrize("two_launches", [False, True], ids=["fused", "two_launches"])
@pytest.mark.parametrize("name,window", [("two", w) for w in windows_of(N_TWO)] + [("mixed", w) for w in windows_of(N_MIXED)])
def test_window_edges(name, window, two_launches, monkeypatch):
    """W = 1, 2, either side of 32 and 64 tie reads (with two candidates each: cells that begin on bit 0, 62 or 2 of a bitmap
    word), the number of tie reads and either side of it, half of it, and 2^31, which is clamped to 2^30: one window"""
    ntie = len(T.tie_rows(T.input_candidates(name)[2]))
    assert ntie == (N_TWO if name == "two" else N_MIXED)
    path = ({"SCALCE_TIE_WINDOW": f"{window}:two_launches" if two_launches else str(window)}, TWO if two_launches else FUSED,
            window, False)
    b = run_case(monkeypatch, name, f"W={window}", path=path)
    if window >= ntie:
        assert b.tie_plan()["windows"] == 1
    if window == 1 << 31:
        assert b.tie_plan()["window"] == WINDOW_CLAMP


@pytest.mark.parametrize("path_name", ["default", "fused", "two_launches", "global", "sequential", "sequential_two"])
@pytest.mark.parametrize("name", ["tie_first_only", "tie_last_only", "no_tie"])
def test_one_tie_read_or_none(name, path_name, monkeypatch):
    """a batch whose only tie read is row 0, one whose only tie read is its last row, one without any"""
    b = run_case(monkeypatch, name, path_name)
    if name == "no_tie":
        assert b.tie_plan()["path"] == 0
    elif path_name != "global":
        assert b.tie_plan()["windows"] == 1


@pytest.mark.parametrize("window", ["1", "1:two_launches"])
def test_windows_of_one_tie_read_each(window, monkeypatch):
    """W = 1 on the input with every candidate count: every window is one read, the last window too"""
    ntie = len(T.tie_rows(T.input_candidates("walk_ten")[2]))
    two = window.endswith("two_launches")
    b = run_case(monkeypatch, "walk_ten", f"W={window}", path=({"SCALCE_TIE_WINDOW": window}, TWO if two else FUSED, 1, False))
    assert b.tie_plan()["windows"] == ntie


# ---- candidate lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_name", ["fused", "sequential"])
@pytest.mark.parametrize("name,counters", [("walk_t7", SEQ_LDS), ("walk_ten", SEQ_LDS), ("walk_anchor_k8", SEQ_GLOBAL)])
def test_candidate_walks(name, counters, path_name, monkeypatch):
    """2, 3 .. 12 distinct cores per read, some twice, tie reads on row 0 and on the last row: the k-mer walk with and without
    the 7-mer table's outputs and the anchor walk list them in order of first appearance (a fifth leaves the registers of
    tie_candidates_pipe_k; the sequential kernel reads a seventh from memory)"""
    b = run_case(monkeypatch, name, path_name)
    if path_name == "sequential":
        assert b.tie_plan()["sequential"] == counters


# ---- the sequential way out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_name", ["sequential", "sequential_two", "sequential_global"])
@pytest.mark.parametrize("name,counters", [("walk_ten", SEQ_LDS), ("seq_patterns", SEQ_LDS_RAISED), ("seq_all8", SEQ_GLOBAL)])
def test_sequential_counter_placements(name, counters, path_name, monkeypatch):
    """the counters of a table of 160 cores, of the golden table's 15 600 and of all 65 536 8-mers: LDS, LDS with the limit
    raised, global memory -- reached from the windows of either launch shape and from the global sweeps"""
    b = run_case(monkeypatch, name, path_name)
    assert b.tie_plan()["sequential"] == counters and b.stats()["tie_fallback"] == 1


def test_sequential_from_global_sweeps_that_need_six(monkeypatch):
    """a read of B and sixteen of "A then B": six global sweeps (tie_ref.jacobi_sweeps), so the first look at four of them
    finds one that moved; left to themselves the sweeps get there too"""
    b = run_case(monkeypatch, "doubling", "sequential_global")
    assert b.tie_plan() == dict(path=GLOBAL, window=0, windows=0, sequential=SEQ_LDS)
    b = run_case(monkeypatch, "doubling", "global")
    assert b.stats()["jacobi_iters"] > 4


# ---- the cap on cells -----------------------------------------------------------------------------------------------------
def test_window_grows_at_64_mi_cells(monkeypatch):
    """4400 tie reads in windows of one would be 68.6 M cells with the golden table's buckets: the window is resized to two"""
    use_path(monkeypatch, {"SCALCE_TIE_WINDOW": "1"})
    t, reads, cands = T.input_candidates("cell_cap")
    ntie = len(T.tie_rows(cands))
    b, bp = tokenize("cell_cap")
    plan, st = b.tie_plan(), b.stats()
    assert st["tie_reads"] == ntie and ntie * len(bp) > T.MAX_CELLS
    assert plan["path"] == FUSED and plan["window"] >= 2 and plan["windows"] * len(bp) <= T.MAX_CELLS, plan
    assert plan["windows"] == -(-ntie // plan["window"]) and plan["window"] == -(-ntie // (T.MAX_CELLS // len(bp)))
    assert st["tie_fallback"] == 0 and plan["sequential"] == 0
    check_tokens(b, bp, *expected("cell_cap", "none", None), "cell cap")
