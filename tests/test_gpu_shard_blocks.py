"""-m gpu: the device building blocks of a sharded run (scalce_sharded_compress, sharded.cpp), each called directly at the
shapes that select its branches -- one process, one GPU, no ranks.  scalce_copy_pieces, scalce_batch_chunk_plan,
scalce_batch_text_offset, scalce_batch_rewindow, scalce_batch_qinput_edges and scalce_batch_set_chunks otherwise only run
inside whole-archive comparisons of 3-process runs, at whatever alignments, piece sizes, tile positions and rewindow
branches those inputs happen to produce.  Every reference here is plain numpy / Python on the host, or a fresh one-shot
Batch of the same library (which test_gpu_parity checks against the oracle); every comparison is byte or integer equality.
The calls follow the order a rank makes them in: append without tokenizing (rows + quality counters), chunk_plan, rewindow,
tokenize, order, emit."""
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

import oraclelib as O
from scalce_amd import host, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PBIN = os.path.join(HERE, "golden", "patterns.bin")
TILE = 16384  # IDX_TILE of the newline index, and the span of one copy_pieces_k workgroup (256 threads x 4 granules x 16 bytes)
ERR_ARG, ERR_FORMAT = r"^\[1\]", r"^\[3\]"


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def dev(data):
    """bytes -> device tensor (16 bytes of nothing for an empty text: the entry points want a pointer)"""
    from gpu_util import device_bytes
    return device_bytes(data if len(data) else bytes(16))


def ptr(t):
    return t.data_ptr()


def make_records(names, bases, quals):
    return [b"@" + nm.encode() + b"\n" + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i, nm in enumerate(names)]


def mixed_names(n, seed):
    """a third of the names longer than a 16-byte cell holds (15 characters), the lengths 14 .. 17 among them"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        stem = "r%d" % i
        if i % 3 == 0:
            out.append(stem + "x" * (int(rng.integers(16, 61)) - len(stem)))
        elif i % 3 == 1:
            out.append(stem + "y" * max(0, int(rng.integers(1, 16)) - len(stem)))
        else:
            out.append(stem)
    for k, ln in enumerate((14, 15, 16, 17)):
        out[5 + k] = ("q%d" % k).ljust(ln, "z")
    return out


Cfg = namedtuple("Cfg", "L paired names nq B")
CFGS = {
    "se100": Cfg(100, False, "short", False, 150_000),
    "pe150": Cfg(150, True, "short", False, 400_000),
    "nonames": Cfg(100, False, "none", False, 150_000),
    "noqual": Cfg(100, False, "short", True, 60_000),
    "se100_mixed": Cfg(100, False, "mixed", False, 150_000),
    "pe150_mixed": Cfg(150, True, "mixed", False, 400_000),
}


@functools.lru_cache(maxsize=None)
def run_records(cfg_name, n):
    """[mate] -> (records, bases, quals) of one longer run; pieces of it are what a rank holds, sends and receives"""
    cfg = CFGS[cfg_name]
    out = []
    for m in range(2 if cfg.paired else 1):
        bases, quals = synth.reads_and_quals(n, cfg.L, seed=700 + 10 * len(cfg_name) + m, dup_frac=0.1, n_frac=0.003)
        if cfg.names == "mixed":
            names = [nm + "/%d" % (m + 1) for nm in mixed_names(n, 11)] if cfg.paired else mixed_names(n, 11)
        else:
            names = [("p.%d/%d" % (i, m + 1)) if cfg.paired else "s.%d" % i for i in range(n)]
        out.append((make_records(names, bases, quals), bases, quals))
    return out


def new_batch(ctx, cfg, nrec, text_bytes, B=None, **kw):
    return host.Batch(ctx, cfg.L, nrec + 8, text_bytes + 64, paired=cfg.paired, read_len2=cfg.L, use_names=cfg.names != "none",
                      no_qualities=cfg.nq, bucket_set_size=cfg.B if B is None else B, **kw)


def first_pass(b, texts):
    """what a rank does with its piece of the input: rows and quality counters, no tie-break yet (sharded.cpp, step 1)"""
    d = [dev(t) for t in texts]
    b.reset()
    used = b.append(ptr(d[0]), len(texts[0]), ptr(d[1]) if len(texts) == 2 else None, len(texts[1]) if len(texts) == 2 else 0,
                    final=True, flags=host.APPEND_NO_TOKENIZE)
    assert list(used)[:len(texts)] == [len(t) for t in texts]
    return d


def remaining_stages(b):
    b.tokenize()
    b.order()
    b.emit()
    b.finish()


def one_shot(ctx, cfg, texts, B=None):
    """the same text through a fresh batch in one piece: the reference of everything behind the ingest"""
    d = [dev(t) for t in texts]
    b = new_batch(ctx, cfg, texts[0].count(b"\n") // 4, max(len(t) for t in texts), B)
    b.front(ptr(d[0]), len(texts[0]), ptr(d[1]) if len(texts) == 2 else None, len(texts[1]) if len(texts) == 2 else 0)
    b.finish()
    return b


def front_outputs(b, cfg):
    """what the stages in front of the coder leave, per the batch's own outputs"""
    out = dict(tokens=b.output(host.OUT_TOKENS, 0, np.int32), perm=b.output(host.OUT_PERM, 0, np.uint32),
               counts=b.output(host.OUT_BUCKET_COUNTS, 0, np.uint64))
    if cfg.names != "none":
        out.update(names=b.output(host.OUT_NAMES, 0), namelen=b.output(host.OUT_NAMELEN, 0))
    for m in range(2 if cfg.paired else 1):
        out["reads%d" % m] = b.output(host.OUT_READS, m)
        if not cfg.nq:
            out["qstream%d" % m] = b.output(host.OUT_QSTREAM, m)
    return {k: v.copy() for k, v in out.items()}


def assert_same_outputs(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert len(got[k]) == len(want[k]), f"{what}: {k} has {len(got[k])} elements, the one-piece batch {len(want[k])}"
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {k} differs first at element {bad[:4]} of {len(want[k])}"


# ---- a. scalce_copy_pieces ---------------------------------------------------------------------------------------------
FILL = 0xA5
GUARD = 64  # bytes around src and dst: copy_pieces_k loads whole aligned granules around src


def copy_and_check(ctx, lens, a, dmis, first_al, rng):
    """Pieces of `lens` bytes, back to back in a src that starts `a` bytes behind a 16-byte boundary, to disjoint ranges of a
    dst that starts `dmis` bytes behind one -- in random order, with gaps -- against dst[pd[p] + i] = src[ps[p] + i] in
    numpy; everything else of the destination tensor (guards, gaps) must keep its fill.  first_al: the address of piece 0's
    destination modulo 16."""
    import torch
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    ps = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    pd = np.zeros(n, dtype=np.int64)
    pos = 0
    for k, gap in zip(rng.permutation(n), rng.integers(0, 24, size=n)):
        pos += int(gap)
        if k == 0:
            pos += (first_al - (dmis + pos)) % 16
        pd[k] = pos
        pos += int(lens[k])
    dst_total = pos
    sbuf = rng.integers(0, 256, size=GUARD + 16 + total + GUARD + 16, dtype=np.uint8)
    t_src = torch.from_numpy(sbuf).to("cuda:0")
    t_dst = torch.full((GUARD + 16 + dst_total + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    assert ptr(t_src) % 16 == 0 and ptr(t_dst) % 16 == 0
    assert (ptr(t_dst) + GUARD + dmis + int(pd[0])) % 16 == first_al
    d_ps, d_pd = torch.from_numpy(ps).to("cuda:0"), torch.from_numpy(pd).to("cuda:0")
    ctx.copy_pieces(ptr(t_src) + GUARD + a, ptr(t_dst) + GUARD + dmis, ptr(d_ps), ptr(d_pd), n, total)
    torch.cuda.synchronize()
    got = t_dst.cpu().numpy()
    want = np.full_like(got, FILL)
    src = sbuf[GUARD + a:GUARD + a + total]
    for p in range(n):
        at = GUARD + dmis + int(pd[p])
        want[at:at + int(lens[p])] = src[int(ps[p]):int(ps[p] + lens[p])]
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0]) - GUARD - dmis
        inside = np.flatnonzero((pd <= i) & (i < pd + lens))
        where = f"piece {int(inside[0])} (src {int(ps[inside[0]])}, {int(lens[inside[0]])} bytes, dst {int(pd[inside[0]])})" if len(inside) else "no piece (guard or gap)"
        raise AssertionError(f"a={a} dmis={dmis} first_al={first_al}: {len(bad)} bytes differ, first at dst offset {i}: {where}")


def sweep_lengths(a, rng):
    """A few hundred pieces: every length 1 .. 40 (twice), lengths around one and four workgroup spans, one piece that ends
    exactly on a span boundary of the address space (offset TILE - a of src), one that starts one byte behind it, pieces
    longer than two spans (a workgroup in the middle of one sees nothing else), a total that is no multiple of 16."""
    small = list(range(1, 41)) * 2 + [int(x) for x in rng.integers(1, 200, size=220)]
    rng.shuffle(small)
    assert sum(small) > TILE + 200
    lens, boundary, split = [], TILE - a, False
    for n in small:
        pos = sum(lens)
        if not split and pos + n >= boundary:
            lens.append(boundary - pos)   # ends exactly on the boundary
            lens.append(1)                # the boundary's own byte: the next piece starts one byte behind it
            if pos + n > boundary:
                lens.append(pos + n - boundary)
            split = True
        else:
            lens.append(n)
    lens += [TILE - 1, TILE, TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1]
    lens += [int(x) for x in rng.integers(1, 41, size=30)]
    lens.append(16 - (sum(lens) + 11) % 16)  # total = 5 modulo 16
    starts = np.concatenate([[0], np.cumsum(lens)])
    assert split and boundary in starts and boundary + 1 in starts and sum(lens) % 16 == 5 and max(lens) > 2 * TILE
    assert set(range(1, 41)) <= set(lens) and 200 < len(lens) < 1000
    return lens


@pytest.mark.parametrize("a", range(16))
def test_copy_pieces_every_alignment(ctx, a):
    """All 16 source misalignments, each with another of the 16 destination misalignments (5a + 3 mod 16 visits them all),
    and piece 0's destination on a 16-byte boundary, on a multiple of 4 that is none, and on an odd address: the three
    store shapes of a whole granule.  Pieces shorter than a granule, piece edges inside granules and pieces across
    workgroup spans take the byte path."""
    rng = np.random.default_rng(900 + a)
    dmis = (5 * a + 3) % 16
    lens = sweep_lengths(a, rng)
    for first_al in (0, (4, 8, 12)[a % 3], (1, 3, 5, 7, 9, 11, 13, 15)[a % 8]):
        copy_and_check(ctx, lens, a, dmis, first_al, rng)


@pytest.mark.parametrize("lens", [[1], [7], [15], [16], [17], [5000], [4, 7], [3, 1, 11], [16, 16], [TILE], [2 * TILE + 3]],
                         ids=lambda v: "x".join(map(str, v)))
def test_copy_pieces_small_lists(ctx, lens):
    """np == 1, totals below one granule, exactly one, and one workgroup span: at every source misalignment, to aligned,
    4-byte aligned and odd destinations"""
    rng = np.random.default_rng(sum(lens))
    for a in range(16):
        for dmis, first_al in ((0, 0), (4, 4), (3, 11), ((a + 9) % 16, (a + 9) % 16)):
            copy_and_check(ctx, lens, a, dmis, first_al, rng)


def test_copy_pieces_nothing_to_do(ctx):
    """no pieces / no bytes: nothing is launched, nothing is written"""
    import torch
    t = torch.full((256,), FILL, dtype=torch.uint8, device="cuda:0")
    z = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    ctx.copy_pieces(ptr(t) + 64, ptr(t) + 128, ptr(z), ptr(z), 0, 0)
    ctx.copy_pieces(ptr(t) + 64, ptr(t) + 128, ptr(z), ptr(z), 1, 0)
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == FILL).all()


# ---- b. scalce_batch_chunk_plan ----------------------------------------------------------------------------------------
def b_rule(sizes, limit, carry_in):
    """The -B rule in a loop (chunk_bounds_k's comment: the running size of the records since the last dump; the read with
    which it reaches -B closes the chunk), begun with `carry_in` bytes in the open chunk -> (rows in front of which a
    chunk begins, bytes left in the open one)."""
    cuts, carry = [], int(carry_in)
    for r, sz in enumerate(sizes):
        carry += int(sz)
        if limit and carry >= limit:
            cuts.append(r + 1)
            carry = 0
    return cuts, carry


def exact_carry(sizes, limit):
    """Only to FIND an input (b_rule says what it must give): a carry_in with which the chunks end exactly with the last
    row, or None when this -B has none.  The first cut decides every later one, so: from which rows does a chunk chain
    end at N, and which carry puts the first cut in front of such a row."""
    S = np.concatenate([[0], np.cumsum(sizes)])
    n = len(sizes)
    nxt = np.searchsorted(S, S[:-1] + limit, side="left")  # the chunk that begins with row s ends in front of row nxt[s]
    ends_at_n = np.zeros(n + 1, dtype=bool)
    for s in range(n - 1, -1, -1):
        ends_at_n[s] = nxt[s] == n or (nxt[s] < n and ends_at_n[nxt[s]])
    for k in range(2, n):
        if S[k] > limit:
            break
        if ends_at_n[k]:
            return int(limit - S[k])
    return None


def record_sizes(ctx, cfg, ref):
    """RecSize per row: 1 (+ name length) + the packed bases without the core + the qualities + mate 2's + 40; core levels
    and name lengths from the one-piece batch `ref` of the same text"""
    pat = ref.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)[:, 0]
    level = {int(p): (0 if int(p) == host.ROOT_CORE or int(p) < 0 else len(ctx.pattern(int(p)))) for p in np.unique(pat)}
    lv = np.array([level[int(p)] for p in pat], dtype=np.int64)
    L = cfg.L
    sz = (1 + ref.output(host.OUT_NAMELEN, 0).astype(np.int64) if cfg.names != "none" else np.ones(len(pat), dtype=np.int64))
    sz = sz + (L - lv + 3) // 4 + (0 if cfg.nq else L)
    if cfg.paired:
        sz = sz + (L + 3) // 4 + (0 if cfg.nq else L)
    return sz + 40


@pytest.mark.parametrize("case", ["se100", "pe150", "nonames", "noqual", "se100_mixed"])
def test_chunk_plan(ctx, case):
    cfg = CFGS[case]
    n = 3000
    recs = run_records(case, n)
    texts = [b"".join(r[0]) for r in recs]
    ref = one_shot(ctx, cfg, texts, B=0)
    sizes = record_sizes(ctx, cfg, ref).tolist()
    if cfg.names != "none" and not cfg.paired:  # (single-end names are stored whole: the length is the text's own)
        want_len = [len(r.split(b"\n", 1)[0]) - 1 for r in recs[0][0]]
        assert ref.output(host.OUT_NAMELEN, 0).tolist() == want_len
        assert (max(want_len) > 15) == (cfg.names == "mixed")
    total = sum(sizes)
    # a -B of about a 14th of the input with which some carry lets the last row close a chunk (carry_out == 0, a cut at N)
    limit = next((lim for lim in range(total // 14, total // 14 + 1000) if exact_carry(sizes, lim) is not None), None)
    assert limit is not None, "no -B within 1000 bytes of a 14th of the input lets a carry end the chunks with the last row: take another seed"
    cuts0, _ = b_rule(sizes, limit, 0)
    assert 5 <= len(cuts0) <= 30
    b = new_batch(ctx, cfg, n, max(len(t) for t in texts), B=limit)
    keep = first_pass(b, texts)  # noqa: F841 - the text stays where it is
    exact = exact_carry(sizes, limit)
    assert b_rule(sizes, limit, exact)[1] == 0 and b_rule(sizes, limit, exact)[0][-1] == n
    # the first call walks the rows and scans the sizes, every later one only redoes the cuts (S_rows == N)
    for carry_in in (0, 1, limit - 1, limit - int(sizes[0]), exact, limit, limit + 5, 0):
        want_cuts, want_carry = b_rule(sizes, limit, carry_in)
        cuts, carry_out = b.chunk_plan(carry_in, 4000)
        print(case, "carry_in", carry_in, "cuts", len(cuts), "carry_out", carry_out)
        assert cuts.tolist() == want_cuts, f"carry_in {carry_in}"
        assert carry_out == want_carry, f"carry_in {carry_in}"
    assert b_rule(sizes, limit, limit - int(sizes[0]))[0][0] == 1
    # cap: exactly the number of cuts -- the whole plan; fewer -- its first `cap` cuts, and ncuts == cap says so (the
    # header: the list may be cut short, carry_out is then the bytes behind the last cut returned)
    S = np.concatenate([[0], np.cumsum(sizes)])
    cuts, carry_out = b.chunk_plan(0, len(cuts0))
    assert cuts.tolist() == cuts0 and carry_out == b_rule(sizes, limit, 0)[1]
    for cap in (len(cuts0) - 1, 3, 1):
        cuts, carry_out = b.chunk_plan(0, cap)
        assert len(cuts) == cap and cuts.tolist() == cuts0[:cap]
        assert carry_out == total - int(S[cuts0[cap - 1]])
    cuts, carry_out = b.chunk_plan(9, 0)
    assert len(cuts) == 0 and carry_out == 9 + total
    # the plan leaves the rows as they were: the rest of the run is the one-piece batch's (with the plan's chunks)
    remaining_stages(b)
    assert_same_outputs(front_outputs(b, cfg), front_outputs(one_shot(ctx, cfg, texts, B=limit), cfg), case)


def test_chunk_plan_uncut_and_empty(ctx):
    cfg = CFGS["se100"]
    recs = run_records("se100", 3000)
    text = b"".join(recs[0][0])
    sizes = record_sizes(ctx, cfg, one_shot(ctx, cfg, [text], B=0))
    total = int(sizes.sum())
    for B in (total + 1, 1 << 40):  # -B larger than the input: no cut, everything is carried on
        b = new_batch(ctx, cfg, 3000, len(text), B=B)
        keep = first_pass(b, [text])  # noqa: F841
        for carry_in in (0, 12345) if B > total + 1 else (0,):
            cuts, carry_out = b.chunk_plan(carry_in, 64)
            assert len(cuts) == 0 and carry_out == carry_in + total
        cuts, carry_out = b.chunk_plan(1, 64)  # total + 1 is reached with the last row; 2^40 is not
        assert (cuts.tolist(), carry_out) == (([3000], 0) if B == total + 1 else ([], total + 1))
    b = new_batch(ctx, cfg, 3000, len(text), B=0)  # -B 0: never spill
    keep = first_pass(b, [text])  # noqa: F841
    cuts, carry_out = b.chunk_plan(77, 64)
    assert len(cuts) == 0 and carry_out == 77 + total
    b = new_batch(ctx, cfg, 100, 1024, B=1000)  # a rank whose piece of the input is empty
    keep = first_pass(b, [b""])  # noqa: F841
    assert b.n_reads == 0
    for carry_in in (0, 999, 5000):
        cuts, carry_out = b.chunk_plan(carry_in, 64)
        assert len(cuts) == 0 and carry_out == carry_in
    with pytest.raises(host.ScalceError, match=ERR_ARG):  # nothing ingested at all
        new_batch(ctx, cfg, 100, 1024, B=1000).chunk_plan(0, 64)


# ---- c. scalce_batch_text_offset ---------------------------------------------------------------------------------------
def padded_records(n, L, seed, targets, tag):
    """n records whose names are padded so that a record begins exactly at every offset in `targets`"""
    bases, quals = synth.reads_and_quals(n, L, seed=seed)
    todo = sorted(targets)
    names, pos = [], 0
    for i in range(n):
        nm = "%s%d" % (tag, i)
        size = len(nm) + 2 * L + 6
        if todo and 0 <= todo[0] - (pos + size) <= 230:  # the NEXT record begins at the target
            nm += "p" * (todo[0] - (pos + size))
            todo.pop(0)
        names.append(nm)
        pos += len(nm) + 2 * L + 6
    assert not todo, todo
    recs = make_records(names, bases, quals)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    assert set(targets) <= set(starts.tolist())
    return recs


def padded_interleaved(n, L1, L2, seed, targets):
    """2n records, mate 1 and mate 2 of a pair in turn, whose names are padded so that a record of mate m + 1 begins exactly
    at offset t of the INTERLEAVED text for every (t, m) in `targets`: the two records in front share the padding (a pair is
    fewer than 400 bytes, so some record of the wanted mate begins within 400 bytes in front of t)"""
    data = [synth.reads_and_quals(n, L, seed=seed + m) for m, L in enumerate((L1, L2))]
    names = ["%s%d" % ("ab"[j % 2], j // 2) for j in range(2 * n)]
    fixed = [2 * (L1, L2)[j % 2] + 6 for j in range(2 * n)]
    assert sum(fixed[:2]) + 2 * 8 <= 400
    for t, m in sorted(targets):
        starts = np.concatenate([[0], np.cumsum([len(nm) + f for nm, f in zip(names, fixed)])])
        j = max(k for k in range(m, 2 * n, 2) if starts[k] <= t)
        need = int(t - starts[j])
        assert j >= 2 and need < 400 and len(names[j - 1]) < 16 and len(names[j - 2]) < 16
        names[j - 1] += "p" * (need // 2)
        names[j - 2] += "p" * (need - need // 2)
    recs = [make_records([names[j]], data[j % 2][0][j // 2:j // 2 + 1], data[j % 2][1][j // 2:j // 2 + 1])[0] for j in range(2 * n)]
    starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).tolist()
    for t, m in targets:
        assert t in starts and starts.index(t) % 2 == m
    return recs


def line_starts(text, lpr=4):
    """offset at which record k of the text begins, for every k whose first byte or end the text holds"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    return [0] + [int(nl[lpr * k - 1]) + 1 for k in range(1, len(nl) // lpr + 1)]


# records that begin at a multiple of the tile (the newline in front is a tile's last byte), one byte behind one (its first
# byte, and the first newline the tile counts), one byte in front of one, and at a multiple of 64 inside a tile (the newline
# is the 64th byte of a ballot group)
TARGETS1 = (TILE, 2 * TILE + 1, 3 * TILE - 1, 4 * TILE + 64 * 37)
TARGETS2 = (TILE + 1, 2 * TILE, 3 * TILE + 64 * 11, 4 * TILE - 1)


def check_offsets(b, mate, text, nrows, lpr=4):
    want = line_starts(text, lpr)
    assert len(want) >= nrows + 1
    got = [b.text_offset(mate, r) for r in range(nrows + 1)]
    bad = [r for r in range(nrows + 1) if got[r] != want[r]]
    assert not bad, f"mate {mate + 1}: rows {bad[:5]}: {[got[r] for r in bad[:5]]}, the text says {[want[r] for r in bad[:5]]}"
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        b.text_offset(mate, nrows + 1)


def test_text_offset_every_row(ctx):
    n, L = 500, 100
    r1 = padded_records(n, L, 31, TARGETS1, "r")
    text = b"".join(r1)
    assert len(text) > 6 * TILE
    b = host.Batch(ctx, L, n + 8, len(text) + 64)
    keep = first_pass(b, [text])  # noqa: F841
    check_offsets(b, 0, text, n)
    assert b.text_offset(0, n) == len(text)
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        b.text_offset(1, 0)  # no such mate
    # a one-piece ingest is a piece as well
    b2 = host.Batch(ctx, L, n + 8, len(text) + 64)
    b2.ingest(0, ptr(keep[0]), len(text))
    check_offsets(b2, 0, text, n)


def test_text_offset_pieces(ctx):
    """The offset refers to the piece ingested last.  The first piece ends inside a record, without a trailing newline:
    its rows are the whole records in front; the second is what was left of it and the rest of the text."""
    n, L = 500, 100
    recs = padded_records(n, L, 33, TARGETS1, "r")
    text = b"".join(recs)
    b = host.Batch(ctx, L, n + 8, len(text) + 64)
    b.reset()
    for cut_in in (57, 1, 2 * L + 9):  # inside the bases, inside the name, inside the qualities of record 300
        b.reset()
        cut = len(b"".join(recs[:300])) + cut_in
        assert text[cut - 1] != 10
        d1 = dev(text[:cut])
        used = b.append(ptr(d1), cut, flags=host.APPEND_NO_TOKENIZE)[0]
        assert used == len(b"".join(recs[:300])) and b.n_reads == 300
        check_offsets(b, 0, text[:cut], 300)
        assert b.text_offset(0, 300) == used
        rest = text[used:]
        d2 = dev(rest)
        b.append(ptr(d2), len(rest), final=True, flags=host.APPEND_NO_TOKENIZE)
        assert b.n_reads == n
        check_offsets(b, 0, rest, n - 300)
        assert b.text_offset(0, n - 300) == len(rest)


def test_text_offset_both_mates(ctx):
    n, L1, L2 = 500, 100, 80
    r1, r2 = padded_records(n, L1, 35, TARGETS1, "a"), padded_records(n, L2, 36, TARGETS2, "b")
    t1, t2 = b"".join(r1), b"".join(r2)
    d1, d2 = dev(t1), dev(t2)
    b = host.Batch(ctx, L1, n + 8, len(t1) + 64, paired=True, read_len2=L2)
    b.reset()
    b.append(ptr(d1), len(t1), ptr(d2), len(t2), final=True, flags=host.APPEND_NO_TOKENIZE)
    check_offsets(b, 0, t1, n)
    check_offsets(b, 1, t2, n)
    assert (b.text_offset(0, n), b.text_offset(1, n)) == (len(t1), len(t2))


def test_text_offset_interleaved(ctx):
    """-i: one text, mate m of row r is its record 2r + m.  Records of either mate begin at the edges of tiles and ballot
    groups of the interleaved text; mate 2 of row n is a line the text does not have (the walk runs off the last tile)."""
    n, L1, L2 = 500, 100, 80
    targets = [(t, 0) for t in TARGETS1] + [(t + 4 * TILE, 1) for t in TARGETS2]
    ti = b"".join(padded_interleaved(n, L1, L2, 37, targets))
    assert len(ti) > 11 * TILE
    di = dev(ti)
    b = host.Batch(ctx, L1, n + 8, len(ti) + 64, paired=True, read_len2=L2, interleaved=True)
    b.ingest(0, ptr(di), len(ti))
    want = line_starts(ti)
    assert len(want) == 2 * n + 1 and want[2 * n] == len(ti)
    for m in (0, 1):
        got = [b.text_offset(m, r) for r in range(n)]
        assert got == want[m:2 * n:2], f"mate {m + 1}"
    assert b.text_offset(0, n) == len(ti)
    assert b.text_offset(1, n) == len(ti)
    for m in (0, 1):
        with pytest.raises(host.ScalceError, match=ERR_ARG):
            b.text_offset(m, n + 1)


# ---- d. scalce_batch_rewindow ------------------------------------------------------------------------------------------
NOWN, OWN0, NRUN = 4000, 400, 7600  # the rank's own piece is records [400, 4400) of a run of 7600
# (records in front, records behind, keep_first, keep_rows)
SCENARIOS = {
    "front_only": (300, 0, 0, NOWN),
    "back_only_kept_from_137": (0, 250, 137, NOWN - 137),
    "both": (300, 200, 50, NOWN - 150),
    "neither_kept_from_123": (0, 0, 123, NOWN - 500),
    "back_only_shortcut_rows_dropped": (0, 250, 0, NOWN - 700),
    "back_only_shortcut_grows": (0, 3000, 0, NOWN),       # rows_bound beyond the token arrays: ensure_keep moves the kept tokens
    "keep_nothing": (150, 170, 0, 0),
    "keep_nothing_from_the_middle": (150, 170, 2000, 0),
    "identity": (0, 0, 0, NOWN),
    "one_row_each": (1, 1, NOWN - 1, 1),
}


# (A walked batch always keeps its first walk: rewindow sizes the token arrays for rows_bound rows before the kept tokens move,
# and no text of rows_bound's bytes holds more records than that -- a record is at least 2 L + 7 bytes.  So the arm that drops
# the tokens, host_ingest.inc "walk_rows = 0", is reached by the walked == False runs alone; no input can reach it walked.)


def rewindow_texts(case, scenario):
    nf, nb, kf, kr = SCENARIOS[scenario]
    recs = [r[0] for r in run_records(case, NRUN)]
    own = [b"".join(r[OWN0:OWN0 + NOWN]) for r in recs]
    front = [b"".join(r[OWN0 - nf:OWN0]) for r in recs]
    back = [b"".join(r[OWN0 + NOWN:OWN0 + NOWN + nb]) for r in recs]
    after = [front[m] + b"".join(recs[m][OWN0 + kf:OWN0 + kf + kr]) + back[m] for m in range(len(recs))]
    return own, front, back, after


def run_rewindow(ctx, cfg, own, front, back, kf, kr, walked):
    b = new_batch(ctx, cfg, NOWN, max(len(t) for t in own))
    keep = [first_pass(b, own)]
    if walked:  # the plan's first walk: the kept rows keep their tokens, only what arrives is walked
        b.chunk_plan(0, 4000)
    stats = [b.output(w, m).copy() for w in (host.OUT_FREQ4, host.OUT_TABLE) for m in range(len(own))]
    df, db = [dev(t) for t in front], [dev(t) for t in back]
    keep += [df, db]
    b.rewindow(kf, kr, [(ptr(d) if len(t) else None, len(t)) for d, t in zip(df, front)],
               [(ptr(d) if len(t) else None, len(t)) for d, t in zip(db, back)])
    after = [b.output(w, m).copy() for w in (host.OUT_FREQ4, host.OUT_TABLE) for m in range(len(own))]
    assert all((x == y).all() for x, y in zip(stats, after)), "rewindow touched the quality statistics"
    return b, stats, keep


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("case", ["se100", "pe150", "nonames", "se100_mixed", "pe150_mixed"])
def test_rewindow_equals_fresh_batch(ctx, case, scenario):
    """[front | kept | back] after rewindow and the remaining stages is what a fresh batch makes of the same text in one
    piece -- with and without the first walk of scalce_batch_chunk_plan in front of the rewindow."""
    cfg = CFGS[case]
    nf, nb, kf, kr = SCENARIOS[scenario]
    own, front, back, after = rewindow_texts(case, scenario)
    want = front_outputs(one_shot(ctx, cfg, after), cfg)
    for walked in (True, False):
        b, stats, keep = run_rewindow(ctx, cfg, own, front, back, kf, kr, walked)  # noqa: F841 - the texts stay where they are
        assert b.n_reads == nf + kr + nb
        remaining_stages(b)
        assert_same_outputs(front_outputs(b, cfg), want, f"{case} {scenario} walked={walked}")
        for m in range(len(own)):  # every record was counted by the rank that ingested it first
            assert (b.output(host.OUT_FREQ4, m) == stats[m]).all()


def test_rewindow_twice_and_oracle(ctx, tmp_path):
    """Two rewindows in a row (the second set of row arrays goes back and forth), long names at both ends; the read and name
    payloads are the reference coder's for the text the batch ends up holding."""
    case = "se100_mixed"
    cfg = CFGS[case]
    recs = run_records(case, NRUN)[0][0]
    own = b"".join(recs[OWN0:OWN0 + NOWN])
    b = new_batch(ctx, cfg, NOWN, len(own))
    keep = [first_pass(b, [own])]
    b.chunk_plan(0, 4000)
    f1, b1 = b"".join(recs[OWN0 - 90:OWN0]), b"".join(recs[OWN0 + NOWN:OWN0 + NOWN + 60])
    d = [dev(f1), dev(b1)]
    b.rewindow(10, NOWN - 30, [(ptr(d[0]), len(f1))], [(ptr(d[1]), len(b1))])
    held = recs[OWN0 - 90:OWN0] + recs[OWN0 + 10:OWN0 + NOWN - 20] + recs[OWN0 + NOWN:OWN0 + NOWN + 60]
    assert b.n_reads == len(held)
    f2, b2 = b"".join(recs[:45]), b"".join(recs[NRUN - 300:])
    d2 = [dev(f2), dev(b2)]
    b.rewindow(20, len(held) - 100, [(ptr(d2[0]), len(f2))], [(ptr(d2[1]), len(b2))])
    held = recs[:45] + held[20:len(held) - 80] + recs[NRUN - 300:]
    assert b.n_reads == len(held)
    remaining_stages(b)
    text = b"".join(held)
    assert_same_outputs(front_outputs(b, cfg), front_outputs(one_shot(ctx, cfg, [text]), cfg), "two rewindows")
    open(tmp_path / "in_1.fq", "wb").write(text)
    O.orc_cli("compress", PBIN, tmp_path / "in_1.fq", tmp_path / "orc", "-B", cfg.B)
    assert open(tmp_path / "orc_1.scalcer", "rb").read()[16:] == b.output(host.OUT_READS, 0).tobytes()
    assert open(tmp_path / "orc_1.scalcen", "rb").read()[9:] == b.output(host.OUT_NAMES, 0).tobytes()


def test_rewindow_errors(ctx):
    cfg = CFGS["se100"]
    recs = run_records("se100", NRUN)[0][0]
    own = b"".join(recs[OWN0:OWN0 + 1000])
    whole = b"".join(recs[:20])
    for which in ("front", "back"):
        for cut in (len(whole) - 57, len(whole) - 1, len(recs[0]) + 3):  # inside the last record, without its newline, inside a name
            b = new_batch(ctx, cfg, 1000, len(own))
            keep = first_pass(b, [own])  # noqa: F841
            d = dev(whole[:cut])
            piece, none = [(ptr(d), cut)], [(None, 0)]
            with pytest.raises(host.ScalceError, match=rf"^\[3\].*rewindow: the {which} text is not whole records"):
                b.rewindow(0, 1000, piece if which == "front" else none, piece if which == "back" else none)
    # behind such an error the batch holds no rows to go on with (the header); started over, it is as good as new
    keep = first_pass(b, [own])  # noqa: F841
    b.chunk_plan(0, 4000)
    d = dev(whole)
    b.rewindow(5, 980, [(ptr(d), len(whole))], [])
    remaining_stages(b)
    text = whole + b"".join(recs[OWN0 + 5:OWN0 + 985])
    assert_same_outputs(front_outputs(b, cfg), front_outputs(one_shot(ctx, cfg, [text]), cfg), "a batch started over")
    b = new_batch(ctx, cfg, 1000, len(own))
    keep = first_pass(b, [own])  # noqa: F841
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        b.rewindow(1, 1000, [], [])  # beyond the rows held: refused before anything moves
    b.rewindow(0, 1000, [], [])
    b.tokenize()
    with pytest.raises(host.ScalceError, match=r"^\[1\].*tokenized already"):
        b.rewindow(0, 1000, [], [])
    # -i: one GPU only
    r2 = run_records("pe150", 64)
    ti = b"".join(x + y for x, y in zip(r2[0][0], r2[1][0]))
    di = dev(ti)
    il = host.Batch(ctx, 150, 72, len(ti) + 64, paired=True, read_len2=150, interleaved=True)
    il.ingest(0, ptr(di), len(ti))
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        il.rewindow(0, 64, [], [])


# ---- e. scalce_batch_qinput_edges --------------------------------------------------------------------------------------
def want_edges(qps):
    """first two and last two symbols of the q' rows, as the entry point reports them"""
    flat = np.concatenate([q.reshape(-1) for q in qps]) if qps else np.zeros(0, dtype=np.uint8)
    if len(flat) >= 2:
        return [int(flat[0]), int(flat[1]), int(flat[-2]), int(flat[-1])]
    if len(flat) == 1:
        return [int(flat[0]), 0, 0, int(flat[0])]
    return [0, 0, 0, 0]


def qprime(bases, quals):
    return O.quality_stream(quals, bases, 33, np.arange(128))[0]


# L = 1 is the shortest read a batch takes; 100 single-end is the fused row (q' | packed bases, 128 bytes apart), 102 and
# a batch told to unfuse keep q' rows back to back, mate 2 of a pair has a stride of its own
@pytest.mark.parametrize("n", [0, 1, 2, 1000])
@pytest.mark.parametrize("layout", ["L1", "L2", "fused100", "unfused100", "plain102", "pair100_80"])
def test_qinput_edges(ctx, layout, n):
    L = {"L1": 1, "L2": 2, "fused100": 100, "unfused100": 100, "plain102": 102, "pair100_80": 100}[layout]
    Ls = [L, 80] if layout == "pair100_80" else [L]
    data = [synth.reads_and_quals(n, Lm, seed=50 + n + m) for m, Lm in enumerate(Ls)]
    texts = [b"".join(make_records(["e%d" % i for i in range(n)], bs, qs)) for bs, qs in data]
    b = host.Batch(ctx, L, n + 8, len(texts[0]) + 64, paired=len(Ls) == 2, read_len2=Ls[-1])
    if layout == "unfused100":
        b.set_fused_rows(False)
    elif layout == "fused100":
        b.set_fused_rows(True)  # (ERR_ARG if the batch had not chosen fused rows by itself)
    else:
        with pytest.raises(host.ScalceError, match=ERR_ARG):
            b.set_fused_rows(True)
    keep = first_pass(b, texts)  # noqa: F841
    assert b.n_reads == n
    for m, (bs, qs) in enumerate(data):
        edge, nsym, read_len = b.qinput_edges(m)
        assert (nsym, read_len) == (n * Ls[m], Ls[m])
        assert edge == want_edges([qprime(bs, qs)]), f"mate {m + 1}"
        qin = b.output(host.OUT_QINPUT, m)  # and the rows themselves, as one array
        assert qin.tobytes() == qprime(bs, qs).tobytes()
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        b.qinput_edges(len(Ls))


@pytest.mark.parametrize("layout", ["fused100", "unfused100", "pair150"])
def test_qinput_edges_after_rewindow(ctx, layout):
    """both ends of the row range changed: the edges are those of the new first and last rows"""
    case = "pe150" if layout == "pair150" else "se100"
    cfg = CFGS[case]
    run = run_records(case, NRUN)
    own = [b"".join(r[0][100:1100]) for r in run]
    front = [b"".join(r[0][:37]) for r in run]
    back = [b"".join(r[0][1200:1263]) for r in run]
    b = new_batch(ctx, cfg, 1000, max(len(t) for t in own))
    if layout == "unfused100":
        b.set_fused_rows(False)
    keep = first_pass(b, own)  # noqa: F841
    df, db = [dev(t) for t in front], [dev(t) for t in back]
    b.rewindow(10, 500, [(ptr(d), len(t)) for d, t in zip(df, front)], [(ptr(d), len(t)) for d, t in zip(db, back)])
    for m, (_, bases, quals) in enumerate(run):
        rows = np.r_[0:37, 110:610, 1200:1263]
        edge, nsym, read_len = b.qinput_edges(m)
        assert (nsym, read_len) == (600 * cfg.L, cfg.L)
        assert edge == want_edges([qprime(bases[rows], quals[rows])]), f"mate {m + 1}"
    # only the back end moved (nothing is copied): the last row is the last one that arrived
    b2 = new_batch(ctx, cfg, 1000, max(len(t) for t in own))
    keep2 = first_pass(b2, own)  # noqa: F841
    b2.rewindow(0, 999, [], [(ptr(d), len(t)) for d, t in zip(db, back)])
    for m, (_, bases, quals) in enumerate(run):
        rows = np.r_[100:1099, 1200:1263]
        assert b2.qinput_edges(m)[0] == want_edges([qprime(bases[rows], quals[rows])]), f"mate {m + 1}"


def test_qinput_edges_without_qualities(ctx):
    cfg = CFGS["noqual"]
    text = b"".join(run_records("noqual", 3000)[0][0][:100])
    b = new_batch(ctx, cfg, 100, len(text))
    keep = first_pass(b, [text])  # noqa: F841
    with pytest.raises(host.ScalceError, match=ERR_ARG):
        b.qinput_edges(0)


# ---- f. scalce_batch_set_chunks ----------------------------------------------------------------------------------------
def staged(ctx, cfg, text, B, starts=None, before_order=None):
    d = dev(text)
    b = new_batch(ctx, cfg, text.count(b"\n") // 4, len(text), B=B)
    b.ingest(0, ptr(d), len(text))
    b.quality()
    b.tokenize()
    if before_order:
        before_order(b)
    if starts is not None:
        b.set_chunks(starts)
    b.order()
    b.emit()
    b.finish()
    return b


def test_set_chunks(ctx):
    case = "se100_mixed"
    cfg = CFGS[case]
    text = b"".join(run_records(case, NRUN)[0][0][:4000])
    plain = one_shot(ctx, cfg, [text], B=0)
    sizes = record_sizes(ctx, cfg, plain)
    limit = int(sizes.sum()) // 9
    cuts, _ = b_rule(sizes, limit, 0)
    starts = [0] + [c for c in cuts if c < 4000]
    assert 5 <= len(starts) <= 30
    ruled = front_outputs(staged(ctx, cfg, text, limit), cfg)
    assert not np.array_equal(ruled["perm"], front_outputs(plain, cfg)["perm"])  # (the chunks do change the order)
    b = staged(ctx, cfg, text, 1 << 40, starts)
    assert b.stats()["chunks"] == len(starts)
    assert_same_outputs(front_outputs(b, cfg), ruled, "explicit starts of the -B rule")
    # starts = [0]: one chunk, which is no chunks
    assert_same_outputs(front_outputs(staged(ctx, cfg, text, 1 << 40, [0]), cfg), front_outputs(plain, cfg), "starts = [0]")
    # 4096 starts are taken, 4097 are not; None clears them: the -B rule is back
    def fill_and_clear(b):
        b.set_chunks(list(range(4096)))
        with pytest.raises(host.ScalceError, match=ERR_ARG):
            b.set_chunks(list(range(4097)))
        b.set_chunks(None)
    assert_same_outputs(front_outputs(staged(ctx, cfg, text, limit, None, fill_and_clear), cfg), ruled, "cleared starts")
    # every row a chunk of its own, as far as 4096 starts go: records in input order inside every bucket
    b = staged(ctx, cfg, text, 0, list(range(4000)))
    perm = b.output(host.OUT_PERM, 0, np.uint32).astype(np.int64)
    pat = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)[:, 0]
    assert sorted(perm.tolist()) == list(range(4000))
    same_bucket = pat[perm][1:] == pat[perm][:-1]
    assert (np.diff(perm)[same_bucket] > 0).all()
