"""--keep-plus restated in plain Python, for the tests: a record's ENTRY from its third line, the entries of a text, the stream
they make, and a text with entries put back.  An entry is b"" for a bare '+', b"=" when the third line behind its '+' equals
the header line behind its '@' (the whole line, name and what follows it), else b"'" and the third line's bytes behind the '+'."""
import struct

import numpy as np


def entry_of(header_line, third_line):
    """header_line, third_line: the record's first and third line, without their newlines"""
    assert third_line[:1] == b"+", "the third line does not begin with '+'"
    body = third_line[1:]
    if not body:
        return b""
    if body == header_line[1:]:
        return b"="
    return b"'" + body


def line_of(header_line, entry):
    """the third line that `entry` stands for, beside this header line"""
    if entry == b"":
        return b"+"
    if entry == b"=":
        return b"+" + header_line[1:]
    assert entry[:1] == b"'" and len(entry) > 1, "malformed entry"   # (an empty literal would be the bare line)
    return b"+" + entry[1:]


def entries(text, interleaved=False):
    """per mate, the entries of the text's records in input order (interleaved: record 2k + m belongs to mate m)"""
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    ents = [entry_of(lines[i], lines[i + 2]) for i in range(0, len(lines), 4)]
    if not interleaved:
        return [ents]
    assert len(ents) % 2 == 0
    return [ents[0::2], ents[1::2]]


def bare(text):
    """the text as the archive keeps it: every third line a bare '+'"""
    lines = text.split(b"\n")
    for i in range(2, len(lines), 4):
        lines[i] = b"+"
    return b"\n".join(lines)


def body(ents, perm=None):
    """the stream's bytes behind its header: entry perm[k] is the k-th, each followed by a newline"""
    order = range(len(ents)) if perm is None else [int(p) for p in perm]
    return b"".join(ents[p] + b"\n" for p in order)


def stream(ents, perm=None):
    order = list(range(len(ents))) if perm is None else [int(p) for p in perm]
    longest = max((len(ents[p]) for p in order), default=0)
    return b"scalce22" + struct.pack("<iiq", 0, longest, len(order)) + (body(ents, perm) if longest else b"")


def insert(text, offsets, ents):
    """A window's records (bare third lines, `offsets`: where each begins and, last, the text's size) with the entries put
    back -> (text, offsets).  A repeat takes the header line as this text holds it."""
    out, new_off = [], [0]
    for r, e in enumerate(ents):
        rec = text[int(offsets[r]):int(offsets[r + 1])]
        lines = rec.split(b"\n")
        assert len(lines) == 5 and lines[4] == b"" and lines[2] == b"+"
        lines[2] = line_of(lines[0], e)
        out.append(b"\n".join(lines))
        new_off.append(new_off[-1] + len(out[-1]))
    return b"".join(out), np.asarray(new_off, dtype=np.uint64)


def restore(text, ents_per_mate, interleaved=False):
    """a whole text of four-line records with bare third lines, the entries of its records put back (per mate, in its order)"""
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    for k in range(len(lines) // 4):
        e = ents_per_mate[k % 2][k // 2] if interleaved else ents_per_mate[0][k]
        lines[4 * k + 2] = line_of(lines[4 * k], e)
    return b"\n".join(lines) + b"\n"
