"""No device: the host side of --digest.  tools/digeststream_check.cpp drives scalce_amd/csrc/digeststream.hpp (the .scalced
layout, every malformed or truncated form with its message, the messages of the check, and the arithmetic that joins CRCs of
pieces against zlib's crc32_combine64 for lengths 0, 1, 2^32 - 1, 2^32, 2^32 + 1, 2^40 and random pairs) as a program of its
own under AddressSanitizer and UBSan; scalce_crc32_combine and scalce_crc32_plan are called through ctypes, the first against
zlib.crc32 of real bytes; the .scalced layout of scalce_amd/format.py is held against the bytes the header documents."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from scalce_amd import format as F
from scalce_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digest_stream_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "digeststream_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "digeststream_check.cpp"), "-o", exe, "-lz"],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "digeststream_check: ok", r.stdout + r.stderr


def test_combine_against_zlib():
    rng = np.random.default_rng(3)
    text = rng.integers(0, 256, size=70000, dtype=np.uint8).tobytes()
    whole = zlib.crc32(text)
    for cut in [0, 1, 15, 16, 17, 4095, 65535, 65536, len(text) - 1, len(text)]:
        a, b = zlib.crc32(text[:cut]), zlib.crc32(text[cut:])
        assert host.crc32_combine(a, b, len(text) - cut) == whole
    # pieces joined in order, as chunks, windows and stripes are
    crc, at = 0, 0
    for n in [0, 1, 7000, 0, 13, 62986]:
        crc = host.crc32_combine(crc, zlib.crc32(text[at:at + n]), n)
        at += n
    assert at == len(text) and crc == whole
    # zeros: the length alone moves the number
    assert host.crc32_combine(zlib.crc32(b"\0" * 5), zlib.crc32(b"\0" * 9), 9) == zlib.crc32(b"\0" * 14)


def test_plan_is_host_arithmetic():
    g, t, s, wgs = host.crc32_plan(0)
    assert (g, wgs) == (16, 0) and t == 1024 * g
    assert host.crc32_plan(1) == (g, t, t, 1)
    assert host.crc32_plan(t) == (g, t, t, 1) and host.crc32_plan(t + 1) == (g, t, t, 2)
    top = host.crc32_plan(1 << 33)[3]
    assert host.crc32_plan(top * t) == (g, t, t, top) and host.crc32_plan(top * t + 1)[2] == 2 * t
    for n in [1 << 20, (1 << 30) + 5, 1 << 33, 1 << 40]:
        g2, t2, s2, w2 = host.crc32_plan(n)
        assert s2 % t == 0 and w2 <= top and w2 * s2 >= n > (w2 - 1) * s2
    with pytest.raises(host.ScalceError):
        host.crc32_plan((1 << 40) + 1)


def test_digest_file_layout():
    raw = F.pack_digest(1, [(1000, 0xCBF43926), (7, 1)])
    assert raw == b"scalce22" + struct.pack("<iiq", 16, 1, 2) + struct.pack("<QII", 1000, 0xCBF43926, 0) + struct.pack("<QII", 7, 1, 0)
    assert F.unpack_digest(raw) == (1, [(1000, 0xCBF43926), (7, 1)])
    assert F.unpack_digest(F.pack_digest(6, [(0, 0)])) == (6, [(0, 0)])
    for bad in [raw[:23], raw[:40], b"x" + raw[1:], raw + b"\0"]:
        with pytest.raises(ValueError):
            F.unpack_digest(bad)
