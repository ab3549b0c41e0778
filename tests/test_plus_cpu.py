"""No device: the host side of --keep-plus.  tests/plus_ref.py (the feature restated in bytes) is held against hand-written
cases; tools/plusstream_check.cpp drives scalce_amd/csrc/plusstream.hpp (header round trip, the P = 0 form, every error string,
the cursor over read callbacks of 1 byte, 7 bytes and everything at once, a stream cut at every byte, malformed entries) as a
program of its own under AddressSanitizer and UBSan; the .scalcep layout of scalce_amd/format.py is held against the bytes the
header documents."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plus_ref as PR
from scalce_amd import format as fmt
from scalce_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rec(header, third=b"+", bases=b"ACGT", quals=b"IIII"):
    return header + b"\n" + bases + b"\n" + third + b"\n" + quals + b"\n"


# (header line, third line, entry)
HAND = [
    (b"@r1", b"+", b""),                                           # bare
    (b"@r1", b"+r1", b"="),                                        # repeat
    (b"@SRR001666.1 071112_SLXA-EAS1_s_7:5:1:817:345 length=36", b"+SRR001666.1 071112_SLXA-EAS1_s_7:5:1:817:345 length=36", b"="),
    (b"@r1 1:N:0", b"+r1", b"'r1"),                                # the name alone is no repeat: the whole line is compared
    (b"@r1", b"+r1 1:N:0", b"'r1 1:N:0"),
    (b"@r1", b"+r2", b"'r2"),                                      # same length, last byte differs
    (b"@r1", b"+r", b"'r"),                                        # one byte shorter
    (b"@r1", b"+r11", b"'r11"),                                    # one byte longer
    (b"@r1", b"+=", b"'="),                                        # a literal that begins with '='
    (b"@r1", b"+'", b"''"),                                        # ... and with the class byte of literals
    (b"@r1", b"+'r1", b"''r1"),
    (b"@=", b"+=", b"="),                                          # a header line that is "=": still a repeat
    (b"@", b"+", b""),                                             # an empty name: the bare line, not a repeat
    (b"@r1", b"+ ", b"' "),
    (b"@r1", b"++", b"'+"),
]


def test_entry_of_hand_written_records():
    for head, third, want in HAND:
        assert PR.entry_of(head, third) == want, (head, third)
        assert PR.line_of(head, want) == third, (head, third)
    for third in (b"", b"r1", b" +", b"@r1"):
        with pytest.raises(AssertionError):
            PR.entry_of(b"@r1", third)


def test_an_empty_literal_cannot_be():
    """b"'" would stand for a '+' with nothing behind it, which is the bare line: entry_of never makes it, line_of refuses it"""
    assert all(PR.entry_of(h, t) != b"'" for h, t, _ in HAND)
    with pytest.raises(AssertionError):
        PR.line_of(b"@r1", b"'")
    for bad in (b"x", b"=x", b"+r1", b" "):
        with pytest.raises(AssertionError):
            PR.line_of(b"@r1", bad)
        with pytest.raises(ValueError, match="malformed entry"):
            fmt.pack_plus([bad])
    with pytest.raises(ValueError, match="malformed entry"):
        fmt.pack_plus([b"'"])


def test_entries_of_a_text_and_back():
    text = b"".join(rec(h, t) for h, t, _ in HAND)
    assert PR.entries(text) == [[e for _, _, e in HAND]]
    kept = PR.bare(text)
    assert kept == b"".join(rec(h) for h, _, _ in HAND)
    assert PR.restore(kept, PR.entries(text)) == text
    off = np.cumsum([0] + [len(rec(h)) for h, _, _ in HAND])
    got, new_off = PR.insert(kept, off, PR.entries(text)[0])
    assert got == text and list(new_off) == list(np.cumsum([0] + [len(rec(h, t)) for h, t, _ in HAND]))


def test_entries_of_an_interleaved_text():
    pairs = [((b"@p1/1", b"+p1/1"), (b"@p1/2", b"+")), ((b"@p2/1", b"+"), (b"@p2/2", b"+x")), ((b"@p3/1", b"+p3/2"), (b"@p3/2", b"+p3/2"))]
    text = b"".join(rec(*a) + rec(*b) for a, b in pairs)
    assert PR.entries(text, interleaved=True) == [[b"=", b"", b"'p3/2"], [b"", b"'x", b"="]]
    assert PR.restore(PR.bare(text), PR.entries(text, interleaved=True), interleaved=True) == text
    with pytest.raises(AssertionError):
        PR.entries(text + rec(b"@odd"), interleaved=True)


def test_a_repeat_takes_the_header_line_as_it_is_written():
    """-d -n or --no-comments: the header line that goes out differs from the input's, and the repeat follows it"""
    kept = rec(b"@lib.7")
    assert PR.insert(kept, [0, len(kept)], [b"="])[0] == rec(b"@lib.7", b"+lib.7")


def test_stream_for_a_permutation_and_the_form_without_entries():
    ents = [b"=", b"", b"'abc", b"'="]
    assert PR.body(ents) == b"=\n\n'abc\n'=\n"
    assert PR.body(ents, [2, 0, 3, 1]) == b"'abc\n=\n'=\n\n"
    data = PR.stream(ents, [2, 0, 3, 1])
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (0, 4, 4) and data[24:] == b"'abc\n=\n'=\n\n"
    # P = 0: the file is its 24-byte header
    assert PR.stream([b"", b"", b""]) == b"scalce22" + struct.pack("<iiq", 0, 0, 3)
    assert PR.stream([]) == b"scalce22" + struct.pack("<iiq", 0, 0, 0)


# ---- plusstream.hpp under sanitizers --------------------------------------------------------------------------------------------
def test_plus_stream_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plusstream_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "plusstream_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "plusstream_check: ok", r.stdout + r.stderr


def test_plus_stream_header_has_no_hip_include():
    src = open(os.path.join(ROOT, "scalce_amd", "csrc", "plusstream.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", src)


# ---- the layout mirror in format.py ---------------------------------------------------------------------------------------------
def test_plus_stream_layout():
    ents = [b"=", b"", b"'SRR1.1 length=36", b"'="]
    data = fmt.pack_plus(ents)
    assert len(data) == fmt.PLUS_HEADER_BYTES + sum(len(e) + 1 for e in ents)
    assert data[:8] == b"scalce22" and struct.unpack("<iiq", data[8:24]) == (0, 17, 4)
    assert data[24:] == b"=\n\n'SRR1.1 length=36\n'=\n"
    assert data == PR.stream(ents)
    assert fmt.unpack_plus(data) == ents
    none = fmt.pack_plus([b""] * 5)
    assert none == b"scalce22" + struct.pack("<iiq", 0, 0, 5) == PR.stream([b""] * 5) and fmt.unpack_plus(none) == [b""] * 5
    big = fmt.pack_plus([b"'" + b"q" * 65534])
    assert struct.unpack("<iiq", big[8:24]) == (0, 65535, 1) and fmt.unpack_plus(big) == [b"'" + b"q" * 65534]


def test_plus_stream_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        fmt.pack_plus([b"'" + b"q" * 65535])
    with pytest.raises(ValueError):
        fmt.pack_plus([b"'a\nb"])
    good = fmt.pack_plus([b"'ab", b"", b"="])
    for bad, word in ((good[:23], "truncated plus-line stream"), (good[:-1], "truncated plus-line stream"),
                      (good[:-2], "truncated plus-line stream"), (good[:26], "truncated plus-line stream"),
                      (b"notscalc" + good[8:], "is not a scalce plus-line stream"),
                      (good[:8] + struct.pack("<i", 1) + good[12:], "is not a scalce plus-line stream"),
                      (good[:12] + struct.pack("<i", -1) + good[16:], "is not a scalce plus-line stream"),
                      (good[:12] + struct.pack("<i", 65536) + good[16:], "is not a scalce plus-line stream"),
                      (good[:16] + struct.pack("<q", -1) + good[24:], "is not a scalce plus-line stream"),
                      (good[:12] + struct.pack("<i", 2) + good[16:], "an entry is longer than its header says"),
                      (good + b"=\n", "plus-line stream holds 4 entries"),
                      (good[:24] + b"xab" + good[27:], "malformed entry"),
                      (good[:-2] + b"'\n", "malformed entry")):
        with pytest.raises(ValueError, match=word):
            fmt.unpack_plus(bad)


def test_constants_and_structures_are_left_alone():
    assert host.OUT_PLUS == 16 and host.STREAM_KEEP_PLUS == 32
    assert host.OUT_COMMENTS == 14 and host.OUT_EXCEPTIONS == 15 and host.STREAM_KEEP_COMMENTS == 8
    # the option is a setter and a stream flag: no field of the parameter structures
    assert host.Params._fields_[-1][0] == "variable_length"
    assert [f[0] for f in host.UnpackParams._fields_[-3:]] == ["len_rd", "len_user", "len_skip"]


def test_header_declares_the_plus_abi():
    hdr = open(os.path.join(ROOT, "include", "scalce_hip.h")).read()
    for sym in ("scalce_batch_set_keep_plus", "scalce_batch_plus_info", "scalce_fastq_plus_ws_bytes", "scalce_fastq_plus_window",
                "scalce_fastq_plus_pairs_ws_bytes", "scalce_fastq_plus_window_pairs", "scalce_stream_decompress_plus"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert re.search(r"#define\s+SCALCE_STREAM_KEEP_PLUS\s+32\b", hdr)
    assert re.search(r"SCALCE_OUT_PLUS\s*=\s*16\b", hdr)
    assert re.search(r"SCALCE_OUT_COMMENTS\s*=\s*14\b", hdr) and re.search(r"SCALCE_OUT_EXCEPTIONS\s*=\s*15\b", hdr)
