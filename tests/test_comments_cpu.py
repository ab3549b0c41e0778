"""No device: the host side of --keep-comments.  tests/comment_ref.py (the feature restated in bytes) is held against
hand-written cases; tools/commentstream_check.cpp drives scalce_amd/csrc/commentstream.hpp (header round trip, every error
string, the cursor over read callbacks of 1 byte, 7 bytes and everything at once, entries of 0, 1 and 65535 bytes, a stream
cut at every byte) as a program of its own under AddressSanitizer and UBSan; the .scalcec layout of scalce_amd/host.py is
held against the bytes the header documents."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import comment_ref as CR
from scalce_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rec(header, bases=b"ACGT", quals=b"IIII"):
    return header + b"\n" + bases + b"\n+\n" + quals + b"\n"


# ---- comment_ref against cases written by hand --------------------------------------------------------------------------------
HAND = [
    (b"@r1", b""),                              # no space
    (b"@r1 ", b" "),                            # space only
    (b"@r1  x", b"  x"),                        # two spaces in a row
    (b"@ r1 x", b" r1 x"),                      # a space as the first character of the name
    (b"@r\t1 2:N:0", b" 2:N:0"),                # a tab stays part of the name
    (b"@r\t1", b""),
    (b"@", b""),                                # an empty name line
    (b"@SRR1.1 HWI-ST:1:1 length=100", b" HWI-ST:1:1 length=100"),
    (b"@M01:23:000-A1:1:1101:1:2 1:N:0:ATCACG", b" 1:N:0:ATCACG"),
]


def test_entry_of_hand_written_header_lines():
    for line, want in HAND:
        assert CR.entry_of(line) == want, line
    assert CR.entry_of(b"@a ") != CR.entry_of(b"@a")   # the two stay distinct: the round trip is exact


def test_entries_of_a_plain_text():
    text = b"".join(rec(h) for h, _ in HAND)
    assert CR.entries(text) == [[e for _, e in HAND]]
    assert CR.strip(text) == b"".join(rec(h[:len(h) - len(e)]) for h, e in HAND)


def test_entries_of_an_interleaved_text():
    pairs = [(b"@p1 1:N:0:AC", b"@p1 2:N:0:AC"), (b"@p2", b"@p2 2:Y:0"), (b"@p3 ", b"@p3")]
    text = b"".join(rec(a) + rec(b) for a, b in pairs)
    assert CR.entries(text, interleaved=True) == [[b" 1:N:0:AC", b"", b" "], [b" 2:N:0:AC", b" 2:Y:0", b""]]
    with pytest.raises(AssertionError):
        CR.entries(text + rec(b"@odd"), interleaved=True)


def test_entries_of_fasta_and_of_four_line_records():
    fasta = b">s1 first\nACGT\n>s2\nAC\n>s3 \nA\n"
    assert CR.entries(fasta, lines_per_record=2) == [[b" first", b"", b" "]]
    fastq = rec(b"@s1 first") + rec(b"@s2") + rec(b"@s3 ", b"A", b"I")
    assert CR.entries(fastq) == [[b" first", b"", b" "]]
    # a '+' line or a quality line with a space in it is no header line
    assert CR.entries(rec(b"@q", b"AC GT", b"I  II")) == [[b""]]
    with pytest.raises(AssertionError):
        CR.entries(b"@a\nAC\n+\n")


def test_stream_for_a_permutation():
    ents = [b" a", b"", b" ccc", b" "]
    assert CR.body(ents) == b" a\n\n ccc\n \n"
    assert CR.body(ents, [2, 0, 3, 1]) == b" ccc\n a\n \n\n"
    data = CR.stream(ents, [2, 0, 3, 1])
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (0, 4, 4) and data[24:] == b" ccc\n a\n \n\n"
    assert CR.stream([]) == b"scalce22" + struct.pack("<iiq", 0, 0, 0)


def test_window_text_with_entries_put_back():
    stripped = [rec(b"@r1"), rec(b"@r22", b"ACGTA", b"IIIII"), rec(b"@"), b"@f\nACGT\n"]
    ents = [b" 1:N:0", b"", b" ", b" x y"]
    text = b"".join(stripped[:3])
    off = np.cumsum([0] + [len(r) for r in stripped[:3]])
    got, new_off = CR.insert(text, off, ents[:3])
    assert got == rec(b"@r1 1:N:0") + rec(b"@r22", b"ACGTA", b"IIIII") + rec(b"@ ")
    assert list(new_off) == [0, len(rec(b"@r1 1:N:0")), len(rec(b"@r1 1:N:0")) + len(stripped[1]), len(got)]
    got, new_off = CR.insert(stripped[3], [0, len(stripped[3])], ents[3:], lines_per_record=2)
    assert got == b"@f x y\nACGT\n" and list(new_off) == [0, len(got)]
    # the round trip: strip, then insert the text's own entries
    whole = b"".join(rec(h) for h, _ in HAND)
    bare = CR.strip(whole)
    lens = [len(rec(h)) - len(e) for h, e in HAND]
    assert CR.insert(bare, np.cumsum([0] + lens), CR.entries(whole)[0])[0] == whole


# ---- commentstream.hpp under sanitizers -----------------------------------------------------------------------------------------
def test_comment_stream_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "commentstream_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "commentstream_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "commentstream_check: ok", r.stdout + r.stderr


def test_comment_stream_header_has_no_hip_include():
    src = open(os.path.join(ROOT, "scalce_amd", "csrc", "commentstream.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", src)


# ---- the layout mirror in host.py -----------------------------------------------------------------------------------------------
def test_comment_stream_layout():
    ents = [b" 1:N:0:ATCACG", b"", b" ", b" length=100"]
    data = host.pack_comments(ents)
    assert len(data) == host.COMMENT_HEADER_BYTES + sum(len(e) + 1 for e in ents)
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (0, 13, 4)
    assert data[24:] == b" 1:N:0:ATCACG\n\n \n length=100\n"
    assert data == CR.stream(ents)
    assert host.unpack_comments(data) == ents
    assert host.pack_comments([]) == b"scalce22" + struct.pack("<iiq", 0, 0, 0) and host.unpack_comments(host.pack_comments([])) == []
    big = host.pack_comments([b"q" * 65535])
    assert struct.unpack("<iiq", big[8:24]) == (0, 65535, 1) and host.unpack_comments(big) == [b"q" * 65535]


def test_comment_stream_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        host.pack_comments([b"q" * 65536])
    with pytest.raises(ValueError):
        host.pack_comments([b" a\nb"])
    good = host.pack_comments([b" ab", b"", b" c"])
    for bad, word in ((good[:23], "truncated comment stream"), (good[:-1], "truncated comment stream"),
                      (good[:-3], "truncated comment stream"), (good[:26], "truncated comment stream"),
                      (b"notscalc" + good[8:], "is not a scalce comment stream"),
                      (good[:8] + struct.pack("<i", 1) + good[12:], "is not a scalce comment stream"),
                      (good[:8] + struct.pack("<i", 4) + good[12:], "is not a scalce comment stream"),
                      (good[:12] + struct.pack("<i", -1) + good[16:], "is not a scalce comment stream"),
                      (good[:12] + struct.pack("<i", 65536) + good[16:], "is not a scalce comment stream"),
                      (good[:16] + struct.pack("<q", -1) + good[24:], "is not a scalce comment stream"),
                      (good[:12] + struct.pack("<i", 2) + good[16:], "an entry is longer than its header says"),
                      (good + b" d\n", "comment stream holds 4 entries")):
        with pytest.raises(ValueError, match=word):
            host.unpack_comments(bad)


def test_constants_and_structures_are_left_alone():
    assert host.OUT_COMMENTS == 14 and host.STREAM_KEEP_COMMENTS == 8
    assert host.OUT_LENGTHS == 12 and host.OUT_NAMECELLS == 13 and host.STREAM_KEEP_ORDER == 4
    # the option is a setter and a stream flag: no field of the parameter structures
    assert host.Params._fields_[-1][0] == "variable_length"
    assert [f[0] for f in host.UnpackParams._fields_[-3:]] == ["len_rd", "len_user", "len_skip"]
    assert C.sizeof(host.RestoreParams) == 5 * C.sizeof(C.c_void_p)


def test_header_declares_the_comment_abi():
    hdr = open(os.path.join(ROOT, "include", "scalce_hip.h")).read()
    for sym in ("scalce_batch_set_keep_comments", "scalce_batch_comments_info", "scalce_fastq_comment_ws_bytes",
                "scalce_fastq_comment_window"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert re.search(r"#define\s+SCALCE_STREAM_KEEP_COMMENTS\s+8\b", hdr)
    assert re.search(r"SCALCE_OUT_COMMENTS\s*=\s*14\b", hdr)
    assert re.search(r"SCALCE_OUT_LENGTHS\s*=\s*12\b", hdr) and re.search(r"SCALCE_OUT_NAMECELLS\s*=\s*13\b", hdr)
