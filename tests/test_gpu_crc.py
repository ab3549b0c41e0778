"""-m gpu: scalce_crc32_device (kernels_crc.hpp) against zlib.crc32, exact.  G, T, S come from scalce_crc32_plan: bytes per lane
per step, per workgroup step (tile) and per workgroup (span).  Lengths: 0 .. 2G + 1, T - 1 .. T + 1, S - 1 .. S + 1, 2S + 1, and
one that fills the largest grid with full spans and a ragged tail (just under 64 MiB); every length at every start phase 0 .. 15
inside a buffer whose other bytes are 0xA5; random bytes, zeros and 0xFF (zeros: a wrong treatment of the initial value shows
only there); the check value of "123456789"; one 0x80 in a zero buffer at the edges of granule, tile and span; and a launch over
a buffer against scalce_crc32_combine of launches over its two parts, cut at every byte of one tile."""
import zlib

import numpy as np
import pytest
import torch

from scalce_amd import host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5
PAD = 64  # guard bytes in front of and behind every range


@pytest.fixture(scope="module")
def ctx(patterns_blob):
    c = host.Context(0, patterns_bin=patterns_blob)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plan():
    g, t, s, wgs = host.crc32_plan(1)
    assert (g, wgs) == (16, 1) and t % g == 0 and s == t
    return g, t


def big_length(t):
    """the longest range of at most 64 MiB: the plan's largest grid, every workgroup but the last a full span, a ragged tail"""
    n = (64 << 20) - 11
    g, t2, s, wgs = host.crc32_plan(n)
    assert t2 == t and s % t == 0 and s > t and wgs * s >= n > (wgs - 1) * s and n % g != 0
    assert host.crc32_plan(64 << 20)[3] == wgs and host.crc32_plan(1 << 33)[3] == wgs, "not the largest grid"
    return n


def lengths(plan):
    g, t = plan
    s = t
    return sorted(set(list(range(0, 2 * g + 2)) + [t - 1, t, t + 1, s - 1, s, s + 1, 2 * s + 1]))


class Runner:
    """launches collected on the default stream, one read-back"""

    def __init__(self, ctx, slots):
        self.ctx = ctx
        self.out = torch.full((slots,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(host.crc32_ws_bytes(1 << 33), dtype=torch.uint8, device=DEV)
        self.keep, self.k = [], 0

    def add(self, d_buf, off, n):
        assert 0 <= off and off + n <= d_buf.numel()
        host.crc32_device(self.ctx, d_buf.data_ptr() + off, n, self.out.data_ptr() + 4 * self.k, self.ws.data_ptr())
        self.keep.append(d_buf)
        self.k += 1
        return self.k - 1

    def results(self):
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint32)


def guarded(d_data, n, phase):
    """d_data[:n] at start phase `phase` (address % 16) with 0xA5 all around; returns (buffer, offset)"""
    buf = torch.full((n + 2 * PAD + 32,), GUARD, dtype=torch.uint8, device=DEV)
    off = PAD + (phase - (buf.data_ptr() + PAD)) % 16
    assert (buf.data_ptr() + off) % 16 == phase
    buf[off:off + n] = d_data[:n]
    return buf, off


def content(kind, n):
    if kind == "random":
        return np.random.default_rng(7).integers(0, 256, size=n, dtype=np.uint8)
    return np.full(n, 0 if kind == "zeros" else 0xFF, dtype=np.uint8)


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_lengths_and_phases(ctx, plan, kind):
    ls = lengths(plan)
    data = content(kind, max(ls))
    d_data = torch.from_numpy(data).to(DEV)
    run = Runner(ctx, len(ls) * 16)
    want = []
    for n in ls:
        ref = zlib.crc32(data[:n].tobytes())
        for phase in range(16):
            buf, off = guarded(d_data, n, phase)
            run.add(buf, off, n)
            want.append((n, phase, ref))
    got = run.results()
    bad = [(n, ph, hex(ref), hex(int(g))) for (n, ph, ref), g in zip(want, got) if ref != int(g)]
    assert not bad, bad[:8]


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_largest_grid_ragged_tail(ctx, plan, kind):
    n = big_length(plan[1])
    data = content(kind, n)
    ref = zlib.crc32(data.tobytes())
    d_data = torch.from_numpy(data).to(DEV)
    run = Runner(ctx, 16)
    for phase in range(16):   # (one buffer at a time: the stream runs them in order)
        buf, off = guarded(d_data, n, phase)
        run.add(buf, off, n)
        run.keep.clear()
        torch.cuda.synchronize()
    got = run.results()
    assert [hex(int(g)) for g in got] == [hex(ref)] * 16


def test_check_value(ctx):
    d = torch.from_numpy(np.frombuffer(b"123456789", dtype=np.uint8).copy()).to(DEV)
    run = Runner(ctx, 16)
    for phase in range(16):
        buf, off = guarded(d, 9, phase)
        run.add(buf, off, 9)
    assert [hex(int(g)) for g in run.results()] == [hex(0xCBF43926)] * 16


@pytest.mark.parametrize("spans", ["one_tile", "two_tiles"])
def test_single_bit(ctx, plan, spans):
    g, t = plan
    if spans == "one_tile":
        s, n = t, 2 * t + 1
        assert host.crc32_plan(n)[2] == s
    else:   # the shortest grid whose spans hold two tiles; the buffer of S + T + 1 bytes lies at its front
        total = host.crc32_plan(1 << 33)[3] * t + t + 1
        s = host.crc32_plan(total)[2]
        assert s == 2 * t
        n = total
    places = sorted(set([0, g - 1, g, t - 1, t, s - 1, s, s + t, n - 1]))
    run = Runner(ctx, len(places))
    want = []
    for p in places:
        data = np.zeros(n, dtype=np.uint8)
        data[p] = 0x80
        want.append(zlib.crc32(data.tobytes()))
        buf, off = guarded(torch.from_numpy(data).to(DEV), n, 0)
        run.add(buf, off, n)
        run.keep.clear()
        torch.cuda.synchronize()
    assert [hex(int(v)) for v in run.results()] == [hex(w) for w in want]


def test_parts_combine_at_every_byte_of_a_tile(ctx, plan):
    g, t = plan
    n = t + 4099
    data = content("random", n)
    buf, off = guarded(torch.from_numpy(data).to(DEV), n, 3)
    run = Runner(ctx, 2 * (t + 1) + 1)
    whole = run.add(buf, off, n)
    for cut in range(t + 1):
        run.add(buf, off, cut)
        run.add(buf, off + cut, n - cut)
    got = run.results()
    assert int(got[whole]) == zlib.crc32(data.tobytes())
    bad = [cut for cut in range(t + 1)
           if host.crc32_combine(int(got[1 + 2 * cut]), int(got[2 + 2 * cut]), n - cut) != int(got[whole])]
    assert not bad, bad[:8]
    # and the parts themselves, at a few cuts
    for cut in (0, 1, g, t - 1, t):
        assert int(got[1 + 2 * cut]) == zlib.crc32(data[:cut].tobytes())
        assert int(got[2 + 2 * cut]) == zlib.crc32(data[cut:].tobytes())
