"""-m gpu: the coder and decoder kernels at context totals of 2^29 - 1 to 2^32 - 1, on the inputs of tests/coder_totals.py
(each held to its claims by tests/test_coder_totals_cpu.py), against the oracle's coder bit for bit -- no tolerance anywhere.

Which kernel a table selects cannot be observed from outside (but for the lanes coder: Batch.coder_round); it is read from
the host code:
  host_entropy.inc:178  a launch with a context total above 2^29 takes the general step (ac_encode_k<true>,
                        ac_encode_rows_k<true, .>), and at 64 blocks per workgroup falls back to 8: ac_encode_lanes_k runs
                        up to 2^29 only;
  host_entropy.inc:37   the same above 2^30, where the reference's 32-bit intervals start to invert;
  host_decode.inc:76    ac_decode_tight_k when no total exceeds 2^29 and symbol 79 lies outside the span of the symbols that
                        occur, else ac_decode_k.
So the cases at 2^29 - 1 and 2^29 take the plain steps and the tight decoder with the smallest intervals these allow (two
values: D = 1), those at 2^29 + 1 are the first on the other side, 2^30 and 2^30 + 1 stand on both sides of the second
switch with intervals of one value (k = 32 in ac_dec_renorm), top_symbol goes to ac_decode_k whatever its total, and the runs
with SCALCE_AC_DECODE_WPB = 0 take every table that would pick the tight decoder through the plain one as well.
collapse: the encoder follows the reference whether or not the result can be decoded; the decoder is asked for the k symbols
the reference's own decoder still gets right."""
import functools

import numpy as np
import pytest

import coder_totals as T
import oraclelib as O
from gpu_util import In, Out
from scalce_amd import host

pytestmark = pytest.mark.gpu
FRAME = 10 * 1024 * 1024
IDS = ["%s-%d" % c for c in T.CASES]
# SCALCE_AC_BLOCKS_PER_WG, SCALCE_AC_ROUND (the latter where the lanes coder runs: totals up to 2^29)
ENCODER_SHAPES = ((None, None), ("4", None), ("8", None), ("64", None), ("64", "16"), ("64", "32"))
DECODER_WPB = (None, "0", "2", "16")
LANES_MAX_TOTAL = 1 << 29


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    return host.Context(0, patterns_bin=patterns_blob)


def setenv(monkeypatch, **kw):
    for name in ("SCALCE_AC_LANES_USED", "SCALCE_AC_TEST_POISON", "SCALCE_AC_GENERAL", "SCALCE_AC_STRIDE_SCALE", "SCALCE_AC_SLOW_THRESHOLD"):
        monkeypatch.delenv(name, raising=False)
    for name, v in kw.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


@functools.lru_cache(maxsize=None)
def oracle_bytes(name, total):
    c = T.case(name, total)
    return O.AcStat(c.table).encode_stream(c.sym)


def device_stream(sym):
    import torch
    return torch.from_numpy(np.concatenate([sym, np.zeros(64, np.uint8)])).to("cuda:0")


def device_table(table):
    import torch
    return torch.from_numpy(table.view(np.int32)).to("cuda:0")


def encode(ctx, d_tab, d_sym, nsym):
    """-> (the batch, open: its output lives in it; the framed stream on the host)"""
    b = host.Batch(ctx, 100, max_reads=1024, max_text=1 << 20)
    b.entropy_stream(0, d_tab.data_ptr(), d_sym.data_ptr(), nsym)
    b.finish()
    return b, b.output(host.OUT_QUAL, 0).copy()


def same_bytes(enc, want, what):
    assert len(enc) == len(want), f"{what}: {len(enc)} vs {len(want)} bytes"
    bad = np.flatnonzero(enc != want)
    assert len(bad) == 0, f"{what}: coder bytes differ from the oracle's first at byte {bad[:3]} of {len(want)}"


def same_symbols(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{what}: decoded symbols differ first at {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"


# ---- encoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,total", T.CASES, ids=IDS)
def test_encoder_writes_the_oracles_bytes(name, total, ctx, monkeypatch):
    """every case through Batch.entropy_stream in every launch shape: one block per workgroup (ac_encode_k), 4 and 8
    (ac_encode_rows_k), 64 (ac_encode_lanes_k at either round length up to 2^29, the fall-back to 8 above)"""
    c = T.case(name, total)
    want = oracle_bytes(name, total)
    d_tab, d_sym = device_table(c.table), device_stream(c.sym)
    for bpw, rnd in ENCODER_SHAPES:
        if rnd and total > LANES_MAX_TOTAL:
            continue
        setenv(monkeypatch, SCALCE_AC_BLOCKS_PER_WG=bpw, SCALCE_AC_ROUND=rnd)
        b, enc = encode(ctx, d_tab, d_sym, len(c.sym))
        lanes_round = b.coder_round
        b.close()
        same_bytes(enc, want, f"{name} at {total}, {bpw or 1} blocks per workgroup, round {rnd}")
        if bpw == "64":   # the lanes coder ran, or it did not: what host_entropy.inc:178 decides
            assert (lanes_round != 0) == (total <= LANES_MAX_TOTAL), (total, lanes_round)
            assert not rnd or lanes_round == int(rnd)
        else:
            assert lanes_round == 0


# ---- decoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,total", T.CASES, ids=IDS)
def test_decoder_returns_the_symbols(name, total, ctx, monkeypatch):
    """the oracle's bytes through scalce_ac_decoder_launch in every workgroup shape of the tight decoder and through the plain
    one; frames at an odd address with 64 bytes that are not zero behind them, the output between guard bytes.  collapse:
    the first k symbols of the frame, no further"""
    c = T.case(name, total)
    coded = oracle_bytes(name, total).tobytes()
    n = c.k if name == "collapse" else len(c.sym)
    assert name != "collapse" or 64 <= n < len(c.sym)
    for wpb in DECODER_WPB:
        setenv(monkeypatch, SCALCE_AC_DECODE_WPB=wpb)
        dec = ctx.ac_decoder(c.table)
        frames, out = In(coded, 1), Out(n, 3)
        what = f"{name} at {total}, wpb {wpb}"
        assert dec.launch(frames.ptr, frames.nbytes, 1, n, out.ptr) == 0, what
        same_symbols(out.region(what), c.sym[:n], what)
        dec.close()


# ---- device to device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", T.TOTALS)
def test_round_trip_on_the_device(total, ctx, monkeypatch):
    """narrow at every total: the bytes the device coded, where the coder left them, straight into scalce_ac_decode"""
    c = T.case("narrow", total)
    setenv(monkeypatch, SCALCE_AC_BLOCKS_PER_WG=None, SCALCE_AC_ROUND=None, SCALCE_AC_DECODE_WPB=None)
    b, _ = encode(ctx, device_table(c.table), device_stream(c.sym), len(c.sym))
    p, nbytes = b.output_ptr(host.OUT_QUAL, 0)
    out = Out(len(c.sym), 5)
    ctx.ac_decode(c.table, p, nbytes, len(c.sym), out.ptr)
    same_symbols(out.region(f"narrow at {total}"), c.sym, f"narrow at {total}")
    b.close()


# ---- two frames -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_frames(total):
    """narrow's table; FRAME + 12 345 symbols drawn like its random stretch, with crafted stretches at the start of both frames
    (a frame starts the coder afresh and carries its first two symbols raw, as the stretches assume): the case's own in
    front of the first, and the second, 12 345 symbols, is a craft_straddle stretch from its first symbol on.
    -> (case, symbols, the oracle's bytes, device symbols, device table)"""
    c = T.case("narrow", total)
    rng = np.random.default_rng(T.seed_of("two_frames", total))
    sym = T.random_stretch(rng, FRAME + 12_345, c.frequent, T.WEIGHTS, c.rare)
    sym[:c.crafted] = c.sym[:c.crafted]
    sym[FRAME:], maxpend = T.craft_straddle(12_345, T.cum_of(c.table[:T.AC_D]), total, rng, first2=c.frequent[:2], used=c.frequent,
                                            run_max=400)
    assert maxpend > 64
    want = O.AcStat(c.table).encode_stream(sym, threads=2)
    return c, sym, want, device_stream(sym), device_table(c.table)


@pytest.mark.parametrize("bpw", [None, "64"], ids=["1_per_wg", "64_per_wg"])
@pytest.mark.parametrize("total", [2 ** 29, 2 ** 30])
def test_two_frames_encoder(total, bpw, ctx, monkeypatch):
    c, sym, want, d_sym, d_tab = two_frames(total)
    setenv(monkeypatch, SCALCE_AC_BLOCKS_PER_WG=bpw, SCALCE_AC_ROUND=None)
    b, enc = encode(ctx, d_tab, d_sym, len(sym))
    b.close()
    same_bytes(enc, want, f"two frames at {total}, {bpw or 1} blocks per workgroup")


@pytest.mark.parametrize("wpb", [None, "16"], ids=["wpb_default", "wpb_16"])
@pytest.mark.parametrize("total", [2 ** 29, 2 ** 30])
def test_two_frames_decoder(total, wpb, ctx, monkeypatch):
    c, sym, want, _, _ = two_frames(total)
    setenv(monkeypatch, SCALCE_AC_DECODE_WPB=wpb)
    dec = ctx.ac_decoder(c.table)
    frames, out = In(want.tobytes(), 3), Out(len(sym), 41)
    assert dec.launch(frames.ptr, frames.nbytes, 2, len(sym), out.ptr) == 0
    same_symbols(out.region(f"two frames at {total}"), sym, f"two frames at {total}, wpb {wpb}")
    dec.close()


# ---- scaling ----------------------------------------------------------------------------------------------------------------
def counters_for(factor):
    """512000 device counters (the count less the 1 every counter starts with) inside the domain the host guarantees -- the
    scaled count fits 32 bits: counter + 1 < factor * 2^32 --, the edges first: 0, factor - 2, factor - 1, k factor - 1 +- 1,
    2^32 - 1, 2^32, the largest, then random ones of every magnitude"""
    rng = np.random.default_rng(T.seed_of("counters", factor))
    limit = factor * 2 ** 32 - 1          # counters below this
    edges = [0, 1, factor - 2, factor - 1, factor, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, limit - 1, limit - 2,
             factor * (2 ** 32 - 1) - 1, factor * (2 ** 32 - 1), factor * (2 ** 32 - 1) - 2]
    for k in (1, 2, 3, 1000, 2 ** 31, 2 ** 32 - 1):
        edges += [k * factor - 2, k * factor - 1, k * factor]
    edges = sorted({e for e in edges if 0 <= e < limit})
    bits = rng.integers(1, int(limit).bit_length() + 1, size=512000 - len(edges)).astype(np.uint64)
    rest = np.minimum(rng.integers(0, 1 << 62, size=len(bits), dtype=np.uint64) >> (np.uint64(62) - bits), np.uint64(limit - 1))
    return np.concatenate([np.array(edges, dtype=np.uint64), rest]), len(edges)


@pytest.mark.parametrize("factor", [1, 2, 7, 24])
def test_scaling_over_the_whole_domain(factor, ctx):
    """scalce_ac_scale against the oracle's on counts up to factor * 2^32 - 1 (the goldens stop at factor 7 and below 2^32)"""
    import torch
    f4, nedges = counters_for(factor)
    assert len(f4) == 512000 and nedges >= 12 and int(f4.max()) == factor * 2 ** 32 - 2
    want = O.ac_scale(f4 + np.uint64(1), factor)
    assert want.min() >= 1 and int(want.max()) == 2 ** 32 - 1 and (want[:nedges] == 1).any()
    d_f4 = torch.from_numpy(f4.view(np.int64)).to("cuda:0")
    d_tab = torch.full((512000 + 2,), -1, dtype=torch.int32, device="cuda:0")
    ctx.ac_scale(d_f4.data_ptr(), factor, d_tab.data_ptr() + 4)
    torch.cuda.synchronize()
    got = d_tab.cpu().numpy().view(np.uint32)
    assert got[0] == 0xFFFFFFFF and got[-1] == 0xFFFFFFFF, "words beside the table were written"
    bad = np.flatnonzero(got[1:-1] != want)
    assert len(bad) == 0, f"factor {factor}: scaled counts differ at {bad[:4]}: counters {f4[bad[:4]]}, {got[1:-1][bad[:4]]} vs {want[bad[:4]]}"
