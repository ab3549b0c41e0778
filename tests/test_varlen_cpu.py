"""No device: the host side of variable-length runs -- the .scalcel layout of scalce_amd/format.py at both entry widths, and
the rule that picks the read length of a run from the quality sample (scalce_varlen_sample, called without a device like
scalce_range_plan_quality)."""
import ctypes as C
import struct

import numpy as np
import pytest

import varlen_util as V
from scalce_amd import format as F
from scalce_amd import host


# ---- the length stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,width", [(1, 1), (100, 1), (255, 1), (256, 2), (300, 2), (2498, 2)])
def test_length_stream_layout(L, width):
    pad = np.array([0, L, 1, L - 1, L // 2] + list(range(0, L + 1, max(1, L // 7))))
    data = F.pack_lengths(L, pad)
    assert data[:8] == b"scalce22" and struct.unpack("<ii", data[8:16]) == (width, L)
    assert len(data) == 16 + width * len(pad) and F.length_entry_width(L) == width
    body = np.frombuffer(data, dtype="<u%d" % width, offset=16)
    assert (body == pad).all()
    back_L, back = F.unpack_lengths(data)
    assert back_L == L and (back == pad).all()
    assert F.unpack_lengths(F.pack_lengths(L, []))[1].size == 0


def test_length_stream_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        F.pack_lengths(100, [101])
    with pytest.raises(ValueError):
        F.pack_lengths(100, [-1])
    good = F.pack_lengths(300, [0, 300, 17])
    for bad in (good[:15], good[:-1], b"notscalc" + good[8:], good[:8] + struct.pack("<ii", 1, 300) + good[16:],
                good[:16] + struct.pack("<H", 301)):
        with pytest.raises(ValueError):
            F.unpack_lengths(bad)


# ---- L from the sample ------------------------------------------------------------------------------------------------------
def sample_text():
    lens = np.array([30, 0, 77, 12, 100, 5, 64, 99])
    var, _, _ = V.texts(100, lens, 5)
    return lens, var


def test_read_length_is_the_longest_sampled_sequence_line():
    lens, var = sample_text()
    for k in range(1, len(lens) + 1):
        n, L, _ = host.varlen_sample(var, sample=k)
        assert (n, L) == (k, lens[:k].max())
    assert host.varlen_sample(var, sample=100)[:2] == (len(lens), 100)       # the text ends before the sample does
    assert host.varlen_sample(var[:-1], sample=100)[:2] == (len(lens) - 1, lens[:-1].max())  # a record that is cut off is not sampled
    assert host.varlen_sample(b"", sample=5)[:2] == (0, 0)


def test_max_length_overrides_the_sample():
    lens, var = sample_text()
    assert host.varlen_sample(var, sample=3, max_length=150)[:2] == (3, 150)
    assert host.varlen_sample(var, sample=8, max_length=50)[:2] == (8, 50)  # (a read beyond it is the run's error, not the sample's)


def test_histogram_counts_the_quality_characters_that_are_there():
    lens, var = sample_text()
    n, _, stat = host.varlen_sample(var, sample=5)
    want = np.zeros(128, dtype=np.int64)
    for rec in V.records_of(var)[:5]:
        want += np.bincount(np.frombuffer(rec[:-1].split(b"\n")[3], dtype=np.uint8), minlength=128)
    assert n == 5 and (stat == want).all() and stat.sum() == lens[:5].sum()


def test_every_other_record_of_an_interleaved_text():
    lens, var = sample_text()
    assert host.varlen_sample(var, sample=4, stride=2, first=0)[:2] == (4, lens[0::2].max())
    assert host.varlen_sample(var, sample=4, stride=2, first=1)[:2] == (4, lens[1::2].max())


# ---- the structures host.py mirrors -----------------------------------------------------------------------------------------
def test_params_mirror_ends_with_variable_length():
    assert host.Params._fields_[-1][0] == "variable_length"
    assert host.Params.variable_length.offset + 4 <= C.sizeof(host.Params)
    p = host.Params()
    host.lib().scalce_params_default(C.byref(p))
    assert p.variable_length == 0 and p.use_names == 1 and p.qmap[1].offset == 33
    assert [f[0] for f in host.UnpackParams._fields_[-3:]] == ["len_rd", "len_user", "len_skip"]
    assert host.OUT_LENGTHS == 12
