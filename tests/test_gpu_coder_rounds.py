"""ac_encode_lanes_k at both round lengths (SCALCE_AC_ROUND = 16 | 32; kernels_acl.hpp): every case byte for byte against
the oracle's coder on the CPU, never against the other round length.  Rows of up to 48 lanes only -- wider rows have one
length."""
import functools

import numpy as np
import pytest

import oraclelib as O
from scalce_amd import host, synth
from scalce_amd.pipeline import ShardPipeline

pytestmark = pytest.mark.gpu
BLK = 10 * 1024 * 1024
ROUNDS = ["16", "32"]


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def lanes_env(monkeypatch, rnd, lanes=None, poison=None):
    monkeypatch.setenv("SCALCE_AC_BLOCKS_PER_WG", "64")
    monkeypatch.setenv("SCALCE_AC_ROUND", rnd)
    for name, v in (("SCALCE_AC_LANES_USED", lanes), ("SCALCE_AC_TEST_POISON", poison)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def device_stream(sym):
    import torch
    return torch.from_numpy(np.concatenate([sym, np.zeros(64, np.uint8)])).to("cuda:0")


def device_table(table):
    import torch
    return torch.from_numpy(table.view(np.int32)).to("cuda:0")


def encode(ctx, d_tab, d_sym, nsym):
    import os
    b = host.Batch(ctx, 100, max_reads=1024, max_text=1 << 20)
    b.entropy_stream(0, d_tab.data_ptr(), d_sym.data_ptr(), nsym)
    b.finish()
    assert b.coder_round == int(os.environ["SCALCE_AC_ROUND"]), "the launch did not take the round length the switch names"
    enc = b.output(host.OUT_QUAL, 0).copy()
    b.close()
    return enc


def same_bytes(enc, want, what):
    assert len(enc) == len(want), f"{what}: {len(enc)} vs {len(want)} bytes"
    bad = np.flatnonzero(enc != want)
    assert len(bad) == 0, f"{what}: coder bytes differ from the oracle's first at byte {bad[:3]} of {len(want)}"


# ---- round edges of one block ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_case():
    """One stream of 97 symbols and a table; a block of n symbols is its first n."""
    rng = np.random.default_rng(97)
    sym = np.clip(np.rint(rng.normal(28, 8, size=97)), 0, 41).astype(np.uint8)
    table = rng.integers(1, 200, size=512000).astype(np.uint32)
    return sym, table, O.AcStat(table)


@pytest.mark.parametrize("rnd", ROUNDS)
@pytest.mark.parametrize("nsym", [1, 2, 3, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 95, 96, 97])
def test_round_edges_of_a_block(nsym, rnd, ctx, monkeypatch):
    """One block of n symbols: the round of the raw symbols alone (1 .. 3; up to 31 at rounds of 32), a tail in every
    position of a round of 32 (33, 34, 47 .. 49, 63, 65, 95, 97) and rounds that are exactly full (32, 64, 96)."""
    lanes_env(monkeypatch, rnd)
    sym, table, stat = edge_case()
    want = stat.encode_stream(sym[:nsym])
    enc = encode(ctx, device_table(table), device_stream(sym[:nsym]), nsym)
    same_bytes(enc, want, f"{nsym} symbols, rounds of {rnd}")


# ---- a short block behind full ones ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def short_block_stream():
    rng = np.random.default_rng(23)
    sym = np.clip(np.rint(rng.normal(28, 8, size=2 * BLK + 45)), 0, 41).astype(np.uint8)
    table = rng.integers(1, 200, size=512000).astype(np.uint32)
    return sym, table, O.AcStat(table), device_stream(sym), device_table(table)


@functools.lru_cache(maxsize=None)
def short_block_want(k):
    sym, _, stat, _, _ = short_block_stream()
    return stat.encode_stream(sym[:2 * BLK + k])


@pytest.mark.parametrize("rnd", ROUNDS)
@pytest.mark.parametrize("lanes", ["1", "2", "28"])
@pytest.mark.parametrize("k", [1, 17, 31, 32, 45])
def test_short_block_behind_full_ones(k, lanes, rnd, ctx, monkeypatch):
    """2 x 10 MiB + k symbols: with 28 lanes the three blocks are lanes of one workgroup that end in different rounds; with 2
    the last workgroup is partly empty and its only block is the short one; with 1 every block has a workgroup."""
    lanes_env(monkeypatch, rnd, lanes=lanes)
    _, _, _, d_sym, d_tab = short_block_stream()
    enc = encode(ctx, d_tab, d_sym, 2 * BLK + k)
    same_bytes(enc, short_block_want(k), f"2 blocks + {k}, {lanes} lanes, rounds of {rnd}")


# ---- the redo path ---------------------------------------------------------------------------------------------------

def straddle_row():
    """A context-free row whose largest symbol occurs and is exactly the upper half of every context: total 2^15, symbol 79
    = [2^14, 2^15).  Coding symbol 79 from the coder's initial state (lo = 0, hi = 2^32 - 1) gives lo = 2^31, hi = 2^32 - 1,
    one bit is shifted out and the state is the initial one again -- so a run that gpu_util.craft_straddle crafted for the
    start of a block, with 79 79 as its two leading symbols, is the same run behind any number of 79s."""
    row = np.ones(80, dtype=np.uint32)
    row[8:40] = 509
    row[8] += 49
    row[79] = 1 << 14
    assert int(row[:79].sum()) == 1 << 14 and int(row.sum()) == 1 << 15
    return row


@functools.lru_cache(maxsize=None)
def straddle_case(offset):
    """Two blocks; the first 40 000 symbols of the stream (behind `offset` symbols that leave the coder's state alone) are
    a craft_straddle run.  -> (device symbols, device table, symbols, the oracle's bytes)"""
    from gpu_util import craft_straddle
    row = straddle_row()
    cum = np.concatenate([[0], np.cumsum(row)])
    rng = np.random.default_rng(41)
    part, maxpend = craft_straddle(40_000, cum, int(cum[-1]), rng, first2=(79, 79))
    assert maxpend > 64
    nsym = BLK + 50_000
    sym = rng.integers(8, 40, size=nsym).astype(np.uint8)
    sym[rng.integers(0, nsym, size=nsym // 100)] = 79   # the topw exit in plain rounds as well: c_hi == total
    sym[:offset] = 79                                   # (the first two are the block's raw symbols)
    sym[offset:offset + len(part)] = part
    table = np.tile(row, 6400)
    want = O.AcStat(table).encode_stream(sym)
    words = np.frombuffer(want[4:4 + 24000].tobytes(), dtype=np.uint32)
    assert (words == 0xFFFFFFFF).sum() > 300 and (words == 0).sum() > 100, "the crafted run is not what it claims to be"
    return device_stream(sym), device_table(table), nsym, want


@pytest.mark.parametrize("rnd", ROUNDS)
@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("poison", ["1", "2", "7"])
def test_redo_path_at_either_round_length(poison, offset, rnd, ctx, monkeypatch):
    """Every round, every second and every seventh forced through the general steps (SCALCE_AC_TEST_POISON) over long
    pending-carry runs that begin in the first (offset 0) or the second half (offset 16) of a round of 32; rounds with
    the largest symbol of a context take the same path unforced."""
    lanes_env(monkeypatch, rnd, poison=poison)
    d_sym, d_tab, nsym, want = straddle_case(offset)
    enc = encode(ctx, d_tab, d_sym, nsym)
    same_bytes(enc, want, f"poison {poison}, run at symbol {offset}, rounds of {rnd}")


# ---- coding in place -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def in_place_shard():
    from gpu_util import device_bytes
    bases, quals = synth.reads_and_quals(200_000, 100, seed=311, dup_frac=0.1)
    fq = synth.fastq_bytes_fast(bases, quals, prefix="p.")
    return bases, quals, device_bytes(fq), len(fq)


@functools.lru_cache(maxsize=None)
def in_place_want(trie):
    from gpu_util import oracle_streams
    bases, quals, _, _ = in_place_shard()
    ref = oracle_streams(trie, bases, quals, 33, None)
    return ref["qp"][ref["perm"]].reshape(-1)


@pytest.mark.parametrize("rnd", ROUNDS)
@pytest.mark.parametrize("overflow", [False, True])
def test_coding_in_place_at_either_round_length(overflow, rnd, patterns_blob, oracle_trie, monkeypatch):
    """200 000 x 100 bp through the front stages and a grouped launch of the lanes coder that writes each block over its own
    symbols: the bytes of the same shard coded into buffers of its own at that round length, which are the oracle's.
    overflow (SCALCE_AC_INPLACE_TEST): a block's output catches up with its input, the shard is run again from its text."""
    import torch
    lanes_env(monkeypatch, rnd)
    ctx = host.Context(0, patterns_bin=patterns_blob)
    _, _, t, nb = in_place_shard()
    n, L = 200_000, 100
    b = host.Batch(ctx, L, n + 8, nb + 64)   # block buffers of its own
    b.compress(t.data_ptr(), nb)
    b.finish()
    own = b.output(host.OUT_QUAL, 0).copy()
    want = O.AcStat(b.output(host.OUT_TABLE, 0, np.uint32)).encode_stream(in_place_want(oracle_trie))
    b.close()
    same_bytes(own, want, f"buffers of its own, rounds of {rnd}")
    if overflow:
        monkeypatch.setenv("SCALCE_AC_INPLACE_TEST", "1")
    ws = host.Workspace(ctx)
    batches = [host.Batch(ctx, L, n + 8, nb + 64, workspace=ws) for _ in range(2)]
    for x in batches:
        x.set_frame_on_demand(True)
        x.set_code_in_place(True)
    got = {}

    def on_retire(slot, batch, tag):
        got[tag] = batch.output(host.OUT_QUAL, 0).copy()

    pipe = ShardPipeline(batches, group=2, on_retire=on_retire)   # one launch over both shards' blocks
    torch.cuda.synchronize()
    for tag in range(2):
        slot, x = pipe.acquire()
        with torch.cuda.stream(pipe.front):
            x.front(t.data_ptr(), nb, None, 0, pipe.front.cuda_stream)
        pipe.submit(slot, tag=tag, flush=(tag == 1))
    pipe.drain()
    assert sorted(got) == [0, 1]
    for tag, enc in got.items():
        same_bytes(enc, want, f"in place (shard {tag}), rounds of {rnd}")
    assert max(x.coder_round for x in batches) == int(rnd), "the grouped launch did not take the round length the switch names"
    reruns = sum(x.reruns for x in batches)
    assert (reruns > 0) == overflow, f"{reruns} shards were run again from their text"
