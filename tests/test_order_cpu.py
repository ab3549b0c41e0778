"""No device: the host side of --keep-order.  tools/orderstream_check.cpp drives scalce_amd/csrc/orderstream.hpp (header round
trip, every error string, entry checks, the stripe plan, the table of the spill's shares up to 65536 stripes) as a program of
its own under AddressSanitizer and UBSan; scalce_order_plan is called through ctypes like scalce_range_plan_quality; the
.scalceo layout of scalce_amd/host.py is held against the bytes the header documents."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from scalce_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 65536


def test_order_stream_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "orderstream_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "orderstream_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "orderstream_check: ok", r.stdout + r.stderr


# ---- scalce_order_plan ------------------------------------------------------------------------------------------------------
def rec_max(L, mates=1, qual=True):
    """the bound of a record's text the window loop uses: its fixed part, a name of up to 255 bytes, 32 to spare, per mate"""
    return mates * ((2 * L + 6 if qual else L + 3) + 255 + 32)


def test_plan_window_below_one_record():
    assert host.order_plan(3000, 1, rec_max(60)) == (1, 3000)
    assert host.order_plan(3000, rec_max(60) - 1, rec_max(60)) == (1, 3000)
    assert host.order_plan(3000, rec_max(60), rec_max(60)) == (1, 3000)
    assert host.order_plan(3000, 2 * rec_max(60), rec_max(60)) == (2, 1500)


def test_plan_window_is_the_archive():
    assert host.order_plan(3000, 3000 * rec_max(60), rec_max(60)) == (3000, 1)
    assert host.order_plan(3000, 1 << 30, rec_max(60)) == ((1 << 30) // rec_max(60), 1)
    assert host.order_plan(3000, 2999 * rec_max(60), rec_max(60)) == (2999, 2)


def test_plan_no_record_and_one():
    assert host.order_plan(0, 1 << 30, rec_max(100)) == ((1 << 30) // rec_max(100), 0)
    assert host.order_plan(0, 1, rec_max(100)) == (1, 0)
    assert host.order_plan(1, 1, rec_max(100)) == (1, 1)
    assert host.order_plan(1, 1 << 30, rec_max(100)) == ((1 << 30) // rec_max(100), 1)


def test_plan_cap_on_the_stripes():
    assert host.order_plan(CAP, 1, 500) == (1, CAP)
    assert host.order_plan(CAP + 1, 1, 500) == (2, (CAP + 2) // 2)
    R, S = host.order_plan(200_000_000, 1 << 20, rec_max(100))   # a window below 1/65536 of the archive
    assert R == -(-200_000_000 // CAP) and S == -(-200_000_000 // R) and S <= CAP and R * rec_max(100) > 1 << 20
    R, S = host.order_plan(0xFFFFFFFF, 1, 1)
    assert S <= CAP and R * S >= 0xFFFFFFFF
    with pytest.raises(host.ScalceError):
        host.order_plan(1 << 32, 1 << 30, 500)    # more records than a u32 entry names
    with pytest.raises(host.ScalceError):
        host.order_plan(10, 1 << 30, 0)


def test_plan_records_of_the_longest_pair():
    """a pair of 2498-base reads is 10 590 bytes of text at the bound: windows below one record, of one, of three, of the archive"""
    rec = rec_max(2498, mates=2)
    assert rec == 2 * (2 * 2498 + 6 + 255 + 32)
    assert host.order_plan(400, 1, rec) == (1, 400)
    assert host.order_plan(400, 3000, rec) == (1, 400)            # less than one record: a record per stripe all the same
    assert host.order_plan(400, rec - 1, rec) == (1, 400)
    assert host.order_plan(400, rec, rec) == (1, 400)
    assert host.order_plan(400, 3 * rec, rec) == (3, 134)
    assert host.order_plan(400, 3 * rec + rec - 1, rec) == (3, 134)
    assert host.order_plan(400, 400 * rec, rec) == (400, 1)
    assert host.order_plan(400, 1 << 30, rec) == ((1 << 30) // rec, 1)
    R, S = host.order_plan(70_000, 3000, rec)                     # more records than stripes under a window below one record
    assert (R, S) == (2, 35_000)
    single = rec_max(2498)
    assert host.order_plan(400, 3000, single) == (1, 400) and host.order_plan(400, 2 * single, single) == (2, 200)


def test_plan_stripe_text_fits_the_window_unless_the_cap_raised_r():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        N = int(rng.integers(0, 1 << int(rng.integers(1, 31))))
        W = int(rng.integers(1, 1 << int(rng.integers(1, 34))))
        rec = rec_max(int(rng.integers(1, 2499)), int(rng.integers(1, 3)), bool(rng.integers(0, 2)))
        R, S = host.order_plan(N, W, rec)
        plain = max(1, W // rec)
        assert R >= 1 and S == -(-N // R) and S <= CAP
        if R != plain:
            assert R > plain and -(-N // plain) > CAP and (R == 1 or -(-N // (R - 1)) > CAP)   # the cap alone raises R, and no further
        elif W >= rec:
            assert R * rec <= W


# ---- the header mirror in host.py -------------------------------------------------------------------------------------------
def test_order_stream_layout():
    perm = np.array([4, 0, 3, 1, 2])
    data = host.pack_order(perm)
    assert len(data) == host.ORDER_HEADER_BYTES + 4 * 5 == 44
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (4, 0, 5)
    assert (np.frombuffer(data, dtype="<u4", offset=24) == perm).all()
    assert (host.unpack_order(data) == perm).all()
    assert host.unpack_order(host.pack_order([])).size == 0
    big = host.pack_order([0xFFFFFFFF])
    assert host.unpack_order(big)[0] == 0xFFFFFFFF


def test_order_stream_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        host.pack_order([-1])
    with pytest.raises(ValueError):
        host.pack_order([1 << 32])
    good = host.pack_order([2, 0, 1])
    for bad, word in ((good[:23], "truncated order stream"), (good[:-1], "truncated order stream"), (good[:-4], "truncated order stream"),
                      (b"notscalc" + good[8:], "is not a scalce order stream"),
                      (good[:8] + struct.pack("<i", 2) + good[12:], "is not a scalce order stream"),
                      (good[:8] + struct.pack("<i", 8) + good[12:], "is not a scalce order stream"),
                      (good[:12] + struct.pack("<i", 1) + good[16:], "is not a scalce order stream"),
                      (good[:16] + struct.pack("<q", -1) + good[24:], "is not a scalce order stream"),
                      (good + b"\0\0\0\0", "order stream holds 4 entries")):
        with pytest.raises(ValueError, match=word):
            host.unpack_order(bad)


def test_restore_structures_mirror_the_header():
    assert [f[0] for f in host.RestoreParams._fields_] == ["order_rd", "order_user", "spill_dir"]
    assert C.sizeof(host.RestoreParams) == 5 * C.sizeof(C.c_void_p)
    assert C.sizeof(host.RestoreStats) == 9 * 8 and host.RestoreStats._fields_[0][0] == "records"
    assert host.STREAM_KEEP_ORDER == 4 and host.OUT_PERM == 6
