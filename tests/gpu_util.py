"""Helpers for the -m gpu parity tests: run the HIP path through the C ABI, fetch every stream."""
import numpy as np

import oraclelib as O
from coder_totals import craft_straddle  # noqa: F401  (on the coder step restated there; its callers import it from here)
from scalce_amd import host, synth


def device_bytes(data):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def hip_compress(ctx, fastq1, L, fastq2=None, L2=0, **kw):
    import torch
    t1 = device_bytes(fastq1)
    t2 = device_bytes(fastq2) if fastq2 is not None else None
    nrec = fastq1.count(b"\n") // 4
    b = host.Batch(ctx, L, max_reads=nrec + 8, max_text=max(len(fastq1), len(fastq2 or b"")) + 64,
                   paired=fastq2 is not None, read_len2=L2, **kw)
    b.compress(t1.data_ptr(), len(fastq1), t2.data_ptr() if t2 is not None else None, len(fastq2 or b""))
    b.finish()
    torch.cuda.synchronize()
    b._keep = (t1, t2)
    return b


def oracle_streams(trie, bases, quals, qoff=33, qvals=None, chunk=None, no_ac=False):
    """Everything the oracle says about one mate-1 shard."""
    qvals = np.arange(128) if qvals is None else qvals
    pat, end = trie.tokenize(bases)
    perm = trie.order(bases, pat, end, chunk)
    qp, f4 = O.quality_stream(quals, bases, qoff, qvals, no_ac=no_ac)
    return dict(pat=pat, end=end, perm=perm, qp=qp, f4=f4)


def check_against_oracle(ctx, trie, bases, quals, qoff=33, qvals=None, label=""):
    n, L = bases.shape
    fq = synth.fastq_bytes_fast(bases, quals)
    qm = None if qvals is None else [(qoff, qvals), (qoff, qvals)]
    b = hip_compress(ctx, fq, L, qmap=qm)
    ref = oracle_streams(trie, bases, quals, qoff, qvals)
    st = b.stats()
    tok = b.output(host.OUT_TOKENS, 0, np.int32).reshape(-1, 2)
    bad = np.flatnonzero((tok[:, 0] != ref["pat"]) | (tok[:, 1] != ref["end"]))
    assert len(bad) == 0, f"{label}: {len(bad)} token mismatches, first at read {bad[:5]}: hip {tok[bad[:5]]} " \
                          f"oracle {ref['pat'][bad[:5]]},{ref['end'][bad[:5]]} stats {st}"
    perm = b.output(host.OUT_PERM, 0, np.uint32)
    badp = np.flatnonzero(perm != ref["perm"])
    assert len(badp) == 0, f"{label}: permutation differs at {len(badp)} of {n} positions, first {badp[:5]}"
    qin = b.output(host.OUT_QINPUT, 0).reshape(n, L)
    assert (qin == ref["qp"]).all(), f"{label}: q' mismatch"
    f4 = b.output(host.OUT_FREQ4, 0, np.uint64)
    assert (f4 + 1 == ref["f4"]).all(), f"{label}: trigram table mismatch at {np.flatnonzero(f4 + 1 != ref['f4'])[:5]}"
    table = b.output(host.OUT_TABLE, 0, np.uint32)
    assert (table == O.ac_scale(ref["f4"], 1)).all(), f"{label}: scaled table mismatch"
    qs = b.output(host.OUT_QSTREAM, 0)
    want_qs = ref["qp"][ref["perm"]].reshape(-1)
    assert (qs == want_qs).all(), f"{label}: reordered quality stream mismatch"
    enc = b.output(host.OUT_QUAL, 0)
    want = O.AcStat(table).encode_stream(want_qs)
    assert len(enc) == len(want), f"{label}: AC length {len(enc)} vs {len(want)}"
    neq = np.flatnonzero(enc != want)
    assert len(neq) == 0, f"{label}: AC bytes differ first at {neq[:5]} of {len(want)}"
    return b, ref, st


# ---- device buffers between guard bytes (test_gpu_decode_entries, test_gpu_coder_totals) -------------------------------------
GUARD = 1024
SENT = 0xA5  # no symbol (< 80), no character of a text (< 0x90 with the phred offsets used)
DEV = "cuda:0"


class Out:
    """nbytes of output at `offset` from a 256-byte aligned address, sentinel everywhere, GUARD bytes on both sides"""

    def __init__(self, nbytes, offset=0):
        import torch
        self.t = torch.full((256 + GUARD + 64 + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.start = (-self.t.data_ptr()) % 256 + GUARD + offset
        self.nbytes = nbytes
        self.ptr = self.t.data_ptr() + self.start

    def region(self, what="", sentinel_free=True):
        h = self.t.cpu().numpy()
        assert (h[:self.start] == SENT).all(), f"{what}: bytes in front of the output were written"
        assert (h[self.start + self.nbytes:] == SENT).all(), f"{what}: bytes behind the output were written"
        got = h[self.start:self.start + self.nbytes]
        assert not sentinel_free or not (got == SENT).any(), f"{what}: output bytes were left unwritten"
        return got


class In:
    """data at `offset` from a 256-byte aligned address; the tensor ends `slack` bytes behind it (the slack is not zero)"""

    def __init__(self, data, offset=0, slack=64):
        import torch
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        raw = torch.full((offset + len(a) + slack,), 0xEE, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0  # (the allocator hands out blocks aligned to 512 bytes)
        if len(a):
            raw[offset:offset + len(a)] = torch.from_numpy(a.copy()).to(DEV)
        self.t, self.ptr, self.nbytes = raw, raw.data_ptr() + offset, len(a)


# ---- what the order stage sorts by, restated in numpy from the oracle's tokens (test_gpu_order_emit, test_gpu_scale) ----
_CODE = np.zeros(256, dtype=np.uint64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i   # every other letter counts as A (const.cpp:47-49)
PREFIX_BASES = 16      # PREFIX_DIGITS * 4, kernels_order.hpp
RUN_SMALL_MAX = 32     # kernels_order.hpp


def key16(bases, end):
    """The first 16 bases behind the core, padded with A past the read's end (_POS, reads.cpp:557-558), as one number."""
    n, L = bases.shape
    idx = np.asarray(end, dtype=np.int64)[:, None] + np.arange(PREFIX_BASES)[None, :]
    c = _CODE[bases[np.arange(n)[:, None], np.minimum(idx, L - 1)]] * (idx < L)
    return (c << (2 * (PREFIX_BASES - 1 - np.arange(PREFIX_BASES))).astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def record_sizes(pat, pattern_lens, name_lens, L, L2=0):
    """What a record adds to the open spill chunk (compress.cpp:689-702): name, rotated bases, qualities, mate 2, bin_node."""
    level = np.where(pat >= 0, pattern_lens[np.maximum(pat, 0)], 0)
    sz = 1 + np.asarray(name_lens, dtype=np.int64) + (L - level + 3) // 4 + L + 40
    return sz + ((L2 + 3) // 4 + L2 if L2 else 0)


def chunks_by_rule(sizes, limit):
    """The -B rule (compress.cpp:708-715): the record with which the open chunk reaches `limit` bytes closes it.
    -> (chunk of every record, number of chunks)"""
    n = len(sizes)
    S = np.concatenate([[0], np.cumsum(sizes)])
    chunk = np.zeros(n, dtype=np.int32)
    start = c = 0
    while start < n:
        r = min(int(np.searchsorted(S, S[start] + limit, side="left")), n)   # the chunk is [start, r)
        chunk[start:r] = c
        c += 1
        start = r
    return chunk, c


def runs_in_order(perm, pat, chunk, key):
    """Runs of records that tie on (bucket, chunk, 16-base prefix), along a permutation that has them side by side (any
    order that is sorted by these three: the oracle's).  -> (first position, length) of every run, singles included"""
    p = np.asarray(perm, dtype=np.int64)
    chunk = np.zeros(len(p), dtype=np.int32) if chunk is None else chunk
    same = (pat[p][1:] == pat[p][:-1]) & (chunk[p][1:] == chunk[p][:-1]) & (key[p][1:] == key[p][:-1])
    starts = np.flatnonzero(np.concatenate([[True], ~same]))
    return starts, np.diff(np.append(starts, len(p)))


def order_expectation(bases, pat, end, perm, chunk=None):
    """What scalce_batch_stats must report for this input: (records in runs of two or more = order_run_members, whether a
    run of more than RUN_SMALL_MAX has a member with bases behind the prefix = order_radix_fallback != 0), and the runs."""
    L = bases.shape[1]
    starts, lens = runs_in_order(perm, pat, chunk, key16(bases, end))
    if L <= PREFIX_BASES:   # the prefix is the whole key: no second phase
        return 0, False, starts, lens
    behind = (end + PREFIX_BASES < L)[np.asarray(perm, dtype=np.int64)]
    fallback = any(behind[s:s + n].any() for s, n in zip(starts[lens > RUN_SMALL_MAX], lens[lens > RUN_SMALL_MAX]))
    return int(lens[lens > 1].sum()), fallback, starts, lens
