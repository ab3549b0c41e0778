"""What follows the names (--keep-comments), restated in numpy and bytes: the entries of a text per mate, the comment stream
for a given permutation, and the text of a window with its entries put back.  No device, no library call.

An entry is the bytes of a record's header line from the first space inclusive to the newline exclusive: empty for a line
without a space, b" " for b"@name ".  A tab does not end a name (names.cpp:55)."""
import struct

import numpy as np

HEADER_BYTES = 24
MAX_ENTRY = 65535


def entry_of(header_line):
    """header_line: the line without its newline, '@' (or '>') included"""
    at = header_line.find(b" ", 1)   # (the first byte is the marker: a name begins behind it)
    return b"" if at < 0 else header_line[at:]


def header_lines(text, lines_per_record=4):
    lines = bytes(text).split(b"\n")
    assert lines.pop() == b"", "the text ends with a newline"
    assert len(lines) % lines_per_record == 0, "whole records"
    return lines[::lines_per_record]


def entries(text, lines_per_record=4, interleaved=False):
    """-> [entries of mate 1] (a list of bytes per record, input order), or [mate 1's, mate 2's] for an interleaved text:
    record 2k + m of it is mate m of pair k.  lines_per_record: 4 (FASTQ), 2 (FASTA)."""
    e = [entry_of(h) for h in header_lines(text, lines_per_record)]
    if not interleaved:
        return [e]
    assert len(e) % 2 == 0, "whole pairs"
    return [e[0::2], e[1::2]]


def body(ents, perm=None):
    """The entries in archive order, each followed by a newline: SCALCE_OUT_COMMENTS.  perm[k] = input index of record k."""
    order = range(len(ents)) if perm is None else [int(i) for i in perm]
    return b"".join(ents[i] + b"\n" for i in order)


def stream(ents, perm=None):
    """The bytes of the .scalcec file out of its container: header, then body()."""
    longest = max((len(e) for e in ents), default=0)
    assert longest <= MAX_ENTRY
    return b"scalce22" + struct.pack("<iiq", 0, longest, len(ents)) + body(ents, perm)


def insert(text, record_offsets, ents, lines_per_record=4):
    """A window's records "@name\\n..." with entry k put between record k's name and its newline.
    -> (text, record offsets: len(ents) + 1 entries)"""
    text = bytes(text)
    off = [int(v) for v in record_offsets]
    assert len(off) == len(ents) + 1 and off[-1] <= len(text)
    out, new_off = [], [0]
    for k, e in enumerate(ents):
        rec = text[off[k]:off[k + 1]]
        nl = rec.index(b"\n")
        assert rec.count(b"\n") == lines_per_record
        out.append(rec[:nl] + e + rec[nl:])
        new_off.append(new_off[-1] + len(out[-1]))
    return b"".join(out), np.array(new_off, dtype=np.uint64)


def strip(text, lines_per_record=4):
    """The text without what follows its names: what -d gives without the comment stream (the '+' line is left alone)."""
    lines = bytes(text).split(b"\n")
    assert lines.pop() == b""
    for i in range(0, len(lines), lines_per_record):
        e = entry_of(lines[i])
        if e:
            lines[i] = lines[i][:-len(e)]
    return b"\n".join(lines) + b"\n"
