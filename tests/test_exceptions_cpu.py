"""No device: the host side of --keep-bases.  tests/exception_ref.py (the rule in numpy) is held against records written by hand
and against the reference's own round trip -- live where oracle/_ref/ref_full is built, and from tests/golden/exceptions_ref.npz
everywhere; tools/exceptionstream_check.cpp drives scalce_amd/csrc/exceptionstream.hpp as a program of its own under
AddressSanitizer and UBSan; the .scalcex layout of scalce_amd/host.py is held against the bytes the header documents."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import exception_ref as ER
import filecases as F
import oraclelib as O
from scalce_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def arr(s):
    return np.frombuffer(s, dtype=np.uint8).reshape(1, -1)


def ent(rec, pos, letter, q=0):
    return ord(letter) | (ord(q) if q else 0) << 8 | pos << 16 | rec << 28


# ---- exception_ref against records written by hand --------------------------------------------------------------------------
def one(b, q, offset=33, values=ER.IDENTITY):
    """(plain letter, plain quality, entries) of a read of one base"""
    pl, pq = ER.plain(arr(b), None if q is None else arr(q), offset, values)
    e = ER.entries(arr(b), None if q is None else arr(q), offset, values)
    return pl.tobytes(), None if pq is None else pq.tobytes(), [int(x) for x in e]


def test_one_of_each_kind():
    assert one(b"N", b"!") == (b"N", b"!", [])                               # N with the offset quality: the common case, free
    assert one(b"N", b"#") == (b"N", b"!", [ent(0, 0, "N", "#")])            # the quality the forced symbol lost
    assert one(b"n", b"I") == (b"A", b"I", [ent(0, 0, "n", "I")])            # lower-case n is stored as A
    assert one(b"a", b"I") == (b"A", b"I", [ent(0, 0, "a", "I")])
    assert one(b"R", b"I") == (b"A", b"I", [ent(0, 0, "R", "I")])
    assert one(b"A", b"!") == (b"N", b"!", [ent(0, 0, "A", "!")])            # symbol 0 comes back as N
    assert one(b"A", None) == (b"A", None, [])                               # ... and not without qualities
    assert one(b"N", None) == (b"A", None, [ent(0, 0, "N")])                 # where an N comes back as A
    assert one(b"g", None) == (b"G", None, [ent(0, 0, "g")])
    assert one(b"A", b"@", offset=64) == (b"N", b"@", [ent(0, 0, "A", "@")])  # Phred+64
    assert one(b"N", b"@", offset=64) == (b"N", b"@", [])
    assert one(b"N", b"B", offset=64) == (b"N", b"@", [ent(0, 0, "N", "B")])
    for b in b"ACGT":
        assert one(bytes([b]), b"I") == (bytes([b]), b"I", [])


def test_a_lossy_map_that_merges_qualities_into_the_offset():
    values = ER.IDENTITY.copy()
    values[33:39] = 33                                                         # '!' .. '&' all become '!'
    assert one(b"C", b"&", values=values) == (b"N", b"!", [ent(0, 0, "C", "!")])   # the entry's quality is values[q]
    assert one(b"C", b"'", values=values) == (b"C", b"'", [])
    assert one(b"N", b"&", values=values) == (b"N", b"!", [])                  # an N whose quality maps to the offset is free
    assert one(b"N", b"'", values=values) == (b"N", b"!", [ent(0, 0, "N", "'")])
    assert one(b"t", b"%", values=values) == (b"N", b"!", [ent(0, 0, "t", "!")])


def test_entries_ascend_and_follow_a_permutation():
    bases = np.frombuffer(b"ACnTaCGTACGN", dtype=np.uint8).reshape(3, 4)
    quals = np.frombuffer(b"IIIIIIIIIII#", dtype=np.uint8).reshape(3, 4)
    e = ER.entries(bases, quals)
    assert [int(x) for x in e] == [ent(0, 2, "n", "I"), ent(1, 0, "a", "I"), ent(2, 3, "N", "#")]
    p = ER.entries(bases, quals, perm=[2, 0, 1])
    assert [int(x) for x in p] == [ent(0, 3, "N", "#"), ent(1, 2, "n", "I"), ent(2, 0, "a", "I")]
    assert (np.diff(p.astype(np.int64)) > 0).all() and ER.records_with_one(bases, quals) == 3
    # variable-length reads: nothing behind a read's end
    assert len(ER.entries(bases, quals, lens=[2, 4, 3])) == 1
    pl, pq = ER.plain(bases, quals)
    al, aq = ER.apply(pl, pq, e)
    assert (al == bases).all() and (aq == quals).all()
    recs = [b"@r%d\n" % i + pl[i].tobytes() + b"\n+\n" + pq[i].tobytes() + b"\n" for i in range(3)]
    want = [b"@r%d\n" % i + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i in range(3)]
    assert ER.apply_text(recs, e, 4, True) == want
    assert ER.apply_text([b"@x\nACAT\n"], [ent(7, 2, "n")], 4, False, first=7) == [b"@x\nACnT\n"]


# ---- exception_ref against the reference's round trip -------------------------------------------------------------------------
def names_of(text):
    return text.split(b"\n")[0:-1:4]


def check_round_trip(text, plain_text, lossy):
    """the reference's decompressed text is the prediction for every record (it writes them in the archive's order: records
    are matched by their names), and under -p 0 the entries turn the plain text back into the input"""
    bases, quals = ER.parse(text)
    where = {n: i for i, n in enumerate(names_of(text))}
    assert len(where) == len(bases)
    order = np.array([where[n] for n in names_of(plain_text)])
    assert sorted(order) == list(range(len(bases)))
    got_b, got_q = ER.parse(plain_text)
    off, vals = O.qmap_init(np.bincount(quals.reshape(-1) & 127, minlength=128), lossy)
    want_b, want_q = ER.plain(bases, quals, off, vals)
    assert (got_b == want_b[order]).all() and (got_q == want_q[order]).all()
    e = ER.entries(bases, quals, off, vals, perm=order)
    back_b, back_q = ER.apply(got_b, got_q, e)
    assert (back_b == bases[order]).all() and (back_q == ER.mapped(quals, vals)[order]).all()
    if lossy == 0:
        assert (back_q == quals[order]).all()
    return len(e), int(off), vals


def test_rule_predicts_the_reference_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "exceptions_ref.npz"))
    text = z["input"].tobytes()
    bases, _ = ER.parse(text)
    assert bases.shape == (300, 40) and ((bases >= 65) & (bases <= 122)).all()
    x0, off, vals = check_round_trip(text, z["plain_p0"].tobytes(), 0)
    assert x0 > 300 and off == 33 and (vals == np.arange(128)).all()
    x30, off, vals = check_round_trip(text, z["plain_p30"].tobytes(), 30)
    assert x30 > 300 and off == 33 and (vals != np.arange(128)).any()


@pytest.mark.skipif(not os.path.exists(F.REF_FULL), reason="oracle/_ref/ref_full not built (needs the reference's sources)")
@pytest.mark.parametrize("lossy", [0, 30])
def test_rule_predicts_the_reference_live(lossy, tmp_path):
    import make_exceptions_ref as G
    text = G.generated_text(n=1000, L=50, seed=77 + lossy)
    plain_text = G.reference_round_trip(text, ["-p", str(lossy)] if lossy else [], str(tmp_path))
    assert check_round_trip(text, plain_text, lossy)[0] > 1000


def test_fixture_is_what_its_generator_makes():
    import make_exceptions_ref as G
    z = np.load(os.path.join(ROOT, "tests", "golden", "exceptions_ref.npz"))
    assert z["input"].tobytes() == G.generated_text()


# ---- exceptionstream.hpp under sanitizers ---------------------------------------------------------------------------------------
def test_exception_stream_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "exceptionstream_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "exceptionstream_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "exceptionstream_check: ok", r.stdout + r.stderr


def test_exception_stream_header_has_no_hip_include():
    src = open(os.path.join(ROOT, "scalce_amd", "csrc", "exceptionstream.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", src)


# ---- the layout mirror in host.py -----------------------------------------------------------------------------------------------
def test_exception_stream_layout():
    e = [ent(0, 0, "N", "#"), ent(0, 99, "a", "I"), ent(5, 7, "R", "!"), ent((1 << 36) - 2, 2498, "n")]
    assert e[0] == 0x234E and e[2] == 5 << 28 | 7 << 16 | 0x21 << 8 | 0x52
    assert host.exception_entry(5, 7, ord("R"), ord("!")) == e[2]
    data = host.pack_exceptions(e, 2499, (1 << 36) - 1)
    assert len(data) == host.EXCEPTION_HEADER_BYTES + 8 * 4 == 64
    assert data[:8] == b"scalce22" and struct.unpack("<iiqq", data[8:32]) == (8, 2499, (1 << 36) - 1, 4)
    assert data[32:] == b"".join(struct.pack("<Q", x) for x in e)
    assert data == ER.pack(e, 2499, (1 << 36) - 1)
    L, n, got = host.unpack_exceptions(data)
    assert (L, n, list(got)) == (2499, (1 << 36) - 1, e)
    empty = host.pack_exceptions([], 100, 0)
    assert empty == b"scalce22" + struct.pack("<iiqq", 8, 100, 0, 0) and len(host.unpack_exceptions(empty)[2]) == 0


def test_exception_stream_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError, match="ascending"):
        host.pack_exceptions([ent(1, 0, "n"), ent(0, 0, "n")], 50, 2)
    with pytest.raises(ValueError, match="ascending"):
        host.pack_exceptions([ent(1, 0, "n"), ent(1, 0, "n")], 50, 2)
    with pytest.raises(ValueError, match="ascending"):      # one entry per place: another letter at the same place is no second entry
        host.pack_exceptions([ent(1, 0, "a", "I"), ent(1, 0, "n", "J")], 50, 2)
    good = host.pack_exceptions([ent(0, 3, "n", "I"), ent(2, 49, "N", "#")], 50, 3)
    swapped = good[:32] + good[40:48] + good[32:40]
    for bad, word in ((good[:31], "truncated exception stream"), (good[:-1], "truncated exception stream"), (good[:33], "truncated exception stream"),
                      (b"notscalc" + good[8:], "is not a scalce exception stream"),
                      (good[:8] + struct.pack("<i", 4) + good[12:], "is not a scalce exception stream"),
                      (good[:8] + struct.pack("<i", 0) + good[12:], "is not a scalce exception stream"),
                      (good[:12] + struct.pack("<i", 0) + good[16:], "is not a scalce exception stream"),
                      (good[:12] + struct.pack("<i", 4096) + good[16:], "is not a scalce exception stream"),
                      (good[:16] + struct.pack("<q", -1) + good[24:], "is not a scalce exception stream"),
                      (good[:16] + struct.pack("<q", 1 << 36) + good[24:], "is not a scalce exception stream"),
                      (good[:24] + struct.pack("<q", -1) + good[32:], "is not a scalce exception stream"),
                      (swapped, "exception stream: entries are not in ascending order"),
                      (good[:40] + struct.pack("<Q", ent(0, 3, "t", "J")) + good[48:], "exception stream: entries are not in ascending order"),
                      (good[:12] + struct.pack("<i", 49) + good[16:], "exception stream: an entry lies outside its record"),
                      (good[:16] + struct.pack("<q", 2) + good[24:], "exception stream: an entry lies outside its record")):
        with pytest.raises(ValueError, match=word):
            host.unpack_exceptions(bad)


def test_constants_and_structures_are_left_alone():
    assert host.OUT_EXCEPTIONS == 15 and host.STREAM_KEEP_BASES == 16
    assert host.OUT_COMMENTS == 14 and host.STREAM_KEEP_COMMENTS == 8 and host.OUT_NAMECELLS == 13
    assert host.Params._fields_[-1][0] == "variable_length"
    assert [f[0] for f in host.UnpackParams._fields_[-3:]] == ["len_rd", "len_user", "len_skip"]
    assert C.sizeof(host.UnpackComments) == 4 * C.sizeof(C.c_void_p)


NEW_SYMBOLS = ("scalce_batch_set_keep_bases", "scalce_batch_exceptions_info", "scalce_fastq_exception_window",
               "scalce_fastq_exception_pairs_ws_bytes", "scalce_fastq_exception_window_pairs", "scalce_stream_decompress_exceptions")


def test_header_declares_the_exception_abi_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "scalce_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert re.search(r"#define\s+SCALCE_STREAM_KEEP_BASES\s+16\b", hdr)
    assert re.search(r"SCALCE_OUT_EXCEPTIONS\s*=\s*15\b", hdr) and re.search(r"SCALCE_OUT_COMMENTS\s*=\s*14\b", hdr)
    assert "scalce_unpack_exceptions" in hdr
    lib = host.lib()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
