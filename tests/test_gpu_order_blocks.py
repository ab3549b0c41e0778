"""-m gpu: the three device calls of the order restore driven alone, each against numpy (kernels_restore.hpp).
scalce_records_permute moves variable-length records by a list of sources; scalce_order_group groups a window's records by the
stripe of the output their order entry names; scalce_order_place puts a stripe's records in their places and says when the
entries are no permutation.  Shapes are the smallest at which the paths differ: records shorter and longer than a 16-byte
granule, every source alignment, one record and none, 255 / 256 / 257 records (one block and two), 256 stripes and 257 (one
radix pass and two), and one text that spans many workgroups."""
import numpy as np
import pytest
import torch

from scalce_amd import host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    c = host.Context(0, patterns_bin=patterns_blob)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- scalce_records_permute -------------------------------------------------------------------------------------------------
def run_permute(ctx, lens, source, align=0, seed=0, out_cap=None):
    """records of the sizes `lens` filled with bytes that tell record and position; returns nothing, asserts everything"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    source = np.asarray(source, dtype=np.int64)
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    text = rng.integers(0, 256, size=total, dtype=np.uint8)
    recs = [text[int(off[i]):int(off[i + 1])] for i in range(n)]
    want = np.concatenate([recs[s] for s in source] + [np.zeros(0, np.uint8)])
    want_off = np.concatenate([[0], np.cumsum(lens[source] if n else [])]).astype(np.int64)
    # the source at any of the 16 alignments inside a guarded buffer; the output with a guard behind the text's end
    d_src = torch.full((total + 64 + 16,), GUARD, dtype=torch.uint8, device=DEV)
    base = (-d_src.data_ptr()) % 16 + 16 + align
    d_src[base:base + total] = dev(text)
    cap = len(want) + 48 if out_cap is None else out_cap
    d_out = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device=DEV)
    d_off = torch.full((n + 3,), -1, dtype=torch.int64, device=DEV)
    d_roff = dev(off.view(np.int64))
    d_source = dev(source.astype(np.uint32).view(np.int32)) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(host.records_permute_ws_bytes(n), dtype=torch.uint8, device=DEV)
    assert d_out.data_ptr() % 16 == 0
    host.records_permute(ctx, d_src.data_ptr() + base, d_roff.data_ptr(), n, total, d_source.data_ptr(), d_out.data_ptr(), cap,
                         d_off.data_ptr() + 8, ws.data_ptr())
    torch.cuda.synchronize()
    got, h = d_out.cpu().numpy(), d_off.cpu().numpy()
    assert h[0] == -1 and h[-1] == -1 and (h[1:-1] == want_off).all()
    keep = min(len(want), cap)
    assert (got[:keep] == want[:keep]).all()
    assert (got[keep:] == GUARD).all(), "bytes behind the text's end were touched"
    assert (d_src.cpu().numpy()[base:base + total] == text).all()


def mixed_lengths(n, seed, lo=1, hi=80):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    lens[: min(n, 80)] = np.arange(1, 81)[: min(n, 80)]   # every length 1 .. 80 where n allows
    rng.shuffle(lens)
    return lens


def perms(n, seed):
    rng = np.random.default_rng(seed)
    return {"identity": np.arange(n), "reversal": np.arange(n)[::-1].copy(), "random": rng.permutation(n)}


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_permute_record_counts(n, ctx):
    lens = mixed_lengths(n, 10 + n)
    for k, (name, p) in enumerate(perms(n, n).items()):
        run_permute(ctx, lens, p, seed=k)


@pytest.mark.parametrize("align", range(16))
def test_permute_source_at_every_alignment(align, ctx):
    lens = mixed_lengths(300, 77)
    assert lens.sum() % 16 != 0
    run_permute(ctx, lens, perms(300, 3)["random"], align=align, seed=align)


def test_permute_granules_inside_across_and_over_several_records(ctx):
    # runs of tiny records (a granule covers several), long ones (granules inside), and both in turn
    for k, lens in enumerate(([1] * 100, [3, 5, 2, 7] * 40, [80] * 50, [1, 80, 2, 79, 16, 17, 15, 32, 33, 31] * 20, [16] * 64, [48, 1] * 33)):
        lens = np.array(lens)
        for name, p in perms(len(lens), k).items():
            run_permute(ctx, lens, p, seed=k)
    for total_mod in range(1, 16):   # totals that are no multiple of 16
        lens = np.array([37, 21, total_mod + 6])
        run_permute(ctx, lens, [2, 0, 1], seed=total_mod)


def test_permute_empty_records_among_the_others(ctx):
    lens = np.array([0, 5, 0, 0, 40, 0, 17, 0])
    for name, p in perms(len(lens), 1).items():
        run_permute(ctx, lens, p)
    run_permute(ctx, np.zeros(10, dtype=np.int64), np.arange(10)[::-1])


def test_permute_many_workgroups(ctx):
    n = 20000
    rng = np.random.default_rng(4)
    lens = rng.integers(100, 181, size=n)    # about 140 bytes each: 2.8 MB, some 170 workgroups
    run_permute(ctx, lens, rng.permutation(n), align=5, seed=9)


def test_permute_stops_at_the_output_capacity(ctx):
    lens = mixed_lengths(300, 5)
    total = int(lens.sum())
    run_permute(ctx, lens, perms(300, 8)["random"], out_cap=total - 1000)
    run_permute(ctx, lens, perms(300, 8)["random"], out_cap=(total // 2) // 16 * 16)


# ---- scalce_order_group -----------------------------------------------------------------------------------------------------
def run_group(ctx, index, R, N, S=None):
    index = np.asarray(index, dtype=np.int64)
    n = len(index)
    S = -(-N // R) if S is None else S
    d_index = dev(index.astype(np.uint32).view(np.int32)) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_source = torch.full((n + 2,), -1, dtype=torch.int32, device=DEV)
    d_counts = torch.full((S + 2,), -1, dtype=torch.int32, device=DEV)
    d_bad = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(host.order_group_ws_bytes(n, S), dtype=torch.uint8, device=DEV)
    host.order_group(ctx, d_index.data_ptr(), n, R, N, S, d_source.data_ptr() + 4, d_counts.data_ptr() + 4, d_bad.data_ptr() + 4, ws.data_ptr())
    torch.cuda.synchronize()
    src, cnt, bad = d_source.cpu().numpy(), d_counts.cpu().numpy(), d_bad.cpu().numpy()
    assert src[0] == -1 and src[-1] == -1 and cnt[0] == -1 and cnt[-1] == -1 and bad[0] == 7 and bad[2] == 7
    stripe = np.minimum(index // R, S - 1)
    want = np.argsort(stripe, kind="stable")          # grouped by stripe, the window's order kept inside one
    assert (src[1:-1] == want).all()
    assert (cnt[1:-1] == np.bincount(stripe, minlength=S)).all() and cnt[1:-1].sum() == n
    return int(bad[1])


@pytest.mark.parametrize("n,N,R", [(1, 1, 1), (300, 300, 1), (300, 300, 300), (300, 1000, 7), (2049, 5000, 13), (5000, 70000, 273),
                                   (5000, 70000, 274), (4096, 65536, 1), (100, 1 << 32 - 1, 1 << 17)])
def test_group_by_stripe(n, N, R, ctx):
    rng = np.random.default_rng(n + R)
    index = rng.choice(N, size=n, replace=False) if N < 1 << 20 else rng.integers(0, N, size=n)
    assert run_group(ctx, index, R, N) == 0
    assert run_group(ctx, np.sort(index), R, N) == 0
    assert run_group(ctx, np.sort(index)[::-1], R, N) == 0


def test_group_all_in_one_stripe_and_each_in_its_own(ctx):
    assert run_group(ctx, 700 + np.random.default_rng(1).permutation(100), 100, 3000) == 0      # all in stripe 7
    assert run_group(ctx, np.random.default_rng(2).permutation(257) * 10 + 3, 10, 2570) == 0    # one per stripe, 257 stripes
    assert run_group(ctx, np.random.default_rng(3).permutation(256) * 10 + 3, 10, 2560) == 0    # ... and 256: a single pass
    assert run_group(ctx, [], 10, 2560) == 0
    assert run_group(ctx, [5], 10, 2560) == 0


def test_group_keeps_the_windows_order_inside_a_stripe(ctx):
    # equal stripes many times over, in falling index order: only stability keeps them as they came
    index = np.concatenate([np.arange(999, -1, -1), np.arange(999, -1, -1)])
    assert run_group(ctx, index, 250, 1000) == 0


def test_group_reports_an_index_beyond_the_records(ctx):
    index = np.random.default_rng(4).permutation(1000)
    assert run_group(ctx, index, 30, 1000) == 0
    for at in (0, 500, 999):
        bad = index.copy()
        bad[at] = 1000            # equal to N
        assert run_group(ctx, bad, 30, 1000) != 0
    bad = index.copy()
    bad[3] = 0xFFFFFFFF
    assert run_group(ctx, bad, 30, 1000) != 0


# ---- scalce_order_place -----------------------------------------------------------------------------------------------------
def run_place(ctx, index, base, expect):
    index = np.asarray(index, dtype=np.int64)
    m = len(index)
    d_index = dev(index.astype(np.uint32).view(np.int32)) if m else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_source = torch.full((expect + 2,), 5, dtype=torch.int32, device=DEV)
    d_bad = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    host.order_place(ctx, d_index.data_ptr(), m, base, expect, d_source.data_ptr() + 4, d_bad.data_ptr() + 4)
    torch.cuda.synchronize()
    src, bad = d_source.cpu().numpy(), d_bad.cpu().numpy()
    assert src[0] == 5 and src[-1] == 5 and bad[0] == 7 and bad[2] == 7
    return src[1:-1], int(bad[1])


@pytest.mark.parametrize("base,expect", [(0, 1), (0, 300), (3000, 300), (2700, 37), (1 << 31, 1000), (0xFFFFFFFF - 9, 10)])
def test_place_a_correct_stripe(base, expect, ctx):
    rng = np.random.default_rng(expect)
    p = rng.permutation(expect)
    src, bad = run_place(ctx, base + p, base, expect)
    assert bad == 0 and (src == np.argsort(p)).all()      # src[index_i - base] = i


def test_place_reports_what_is_no_permutation(ctx):
    base, expect = 600, 300
    p = np.random.default_rng(9).permutation(expect) + base
    assert run_place(ctx, p, base, expect)[1] == 0
    dup = p.copy()
    dup[17] = dup[200]                                    # two records claim one place (and one place stays empty)
    assert run_place(ctx, dup, base, expect)[1] != 0
    low = p.copy()
    low[5] = base - 1
    assert run_place(ctx, low, base, expect)[1] != 0
    high = p.copy()
    high[299] = base + expect
    assert run_place(ctx, high, base, expect)[1] != 0
    src, bad = run_place(ctx, p[:-1], base, expect)       # m < expect: a place stays empty, and says so
    assert bad != 0 and src[p[-1] - base] == -1 and (np.delete(src, p[-1] - base) >= 0).all()
    assert run_place(ctx, np.concatenate([p, p[:1]]), base, expect)[1] != 0   # m > expect
    assert run_place(ctx, [], base, 0)[1] == 0
    assert run_place(ctx, [], base, 4)[1] != 0


def test_place_every_stripe_of_a_spill(ctx):
    """the second pass in small: windows of a shuffled text grouped by stripe (numpy), every stripe's records put in their places
    -- the short last stripe among them -- give the text in input order"""
    rng = np.random.default_rng(12)
    N, R = 1000, 64
    lens = rng.integers(1, 200, size=N)
    perm = rng.permutation(N)                              # archive record k is input record perm[k]
    recs = [rng.integers(0, 256, size=int(lens[i]), dtype=np.uint8) for i in range(N)]
    S = -(-N // R)
    spill = [[] for _ in range(S)]                         # per stripe: (entry, record) in spill order
    for w0 in range(0, N, 300):
        idx = perm[w0:w0 + 300]
        order = np.argsort(idx // R, kind="stable")
        for k in order:
            spill[idx[k] // R].append((int(idx[k]), recs[idx[k]]))
    out = []
    for s in range(S):
        entries = np.array([e for e, _ in spill[s]])
        expect = min(R, N - s * R)
        src, bad = run_place(ctx, entries, s * R, expect)
        assert bad == 0
        out += [spill[s][j][1] for j in src]
    assert all((a == b).all() for a, b in zip(out, recs)) and len(out) == N


# ---- scalce_batch_set_keep_order --------------------------------------------------------------------------------------------
def test_lean_batch_keeps_the_permutation_when_asked(ctx):
    from scalce_amd import synth
    bases, quals = synth.reads_and_quals(5000, 60, seed=3, dup_frac=0.2)
    fq = synth.fastq_bytes_fast(bases, quals)
    t = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    perms = {}
    for lean, keep in ((False, False), (True, True), (True, False)):
        b = host.Batch(ctx, 60, 5008, len(fq) + 64)
        b.set_lean(lean)
        if keep:
            b.set_keep_order(True)
        b.compress(t.data_ptr(), len(fq))
        b.finish()
        ptr, nbytes = b.output_ptr(host.OUT_PERM, 0)
        perms[lean, keep] = b.output(host.OUT_PERM, 0, np.uint32).copy() if ptr else None
        b.close()
    assert perms[False, False] is not None and (np.sort(perms[False, False]) == np.arange(5000)).all()
    assert perms[True, True] is not None and (perms[True, True] == perms[False, False]).all()
    assert perms[True, False] is None     # (a lean batch gives the permutation up, as before)
