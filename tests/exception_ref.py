"""The rule of --keep-bases in numpy: what the archive gives back for a read (the PLAIN text), which positions are exceptions,
the bytes of a .scalcex stream, and putting the entries back.

With the input's letter b and quality character q at a position, values[] / offset the run's quality map:
  stored symbol  s = 0 if b == 'N', else values[q] - offset          (runs with qualities only; qualities.cpp:183)
  plain letter   'N' if the run has qualities and s == 0 (decompress.cpp:350-351), else "ACGT"[getval(b)] (const.cpp:47-49)
  plain quality  offset + s
The position is an exception when the plain letter differs from b, or when the run has qualities, b == 'N' and
values[q] != offset.  Its entry carries b and values[q] (0 without qualities)."""
import struct

import numpy as np

IDENTITY = np.arange(128, dtype=np.int64)
_CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i       # getval: a c g t like A C G T, every other byte 0
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
HEADER_BYTES = 32


def parse(text, lines_per_record=4):
    """(bases, quals) of a text of records of ONE read length: n x L uint8 arrays; quals is None for two-line records"""
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) % lines_per_record == 0
    seq = lines[1::lines_per_record]
    L = len(seq[0]) if seq else 0
    bases = np.frombuffer(b"".join(seq), dtype=np.uint8).reshape(len(seq), L)
    if lines_per_record == 2:
        return bases, None
    quals = np.frombuffer(b"".join(lines[3::4]), dtype=np.uint8).reshape(len(seq), L)
    return bases, quals


def mapped(quals, values):
    """values[q] of every quality character (the ingest looks at the low seven bits)"""
    return np.asarray(values, dtype=np.int64)[quals & 127]


def plain(bases, quals=None, offset=33, values=IDENTITY):
    """what -d writes today for these reads: (letters, quality characters or None)"""
    letters = _ACGT[_CODE[bases]]
    if quals is None:
        return letters, None
    s = np.where(bases == ord("N"), 0, mapped(quals, values) - offset)
    return np.where(s == 0, np.uint8(ord("N")), letters), (offset + s).astype(np.uint8)


def exception_mask(bases, quals=None, offset=33, values=IDENTITY, lens=None):
    letters, _ = plain(bases, quals, offset, values)
    m = letters != bases
    if quals is not None:
        m |= (bases == ord("N")) & (mapped(quals, values) != offset)
    if lens is not None:    # variable-length reads: the pad behind a read's end is no part of it
        m &= np.arange(bases.shape[1])[None, :] < np.asarray(lens)[:, None]
    return m


def entries(bases, quals=None, offset=33, values=IDENTITY, perm=None, lens=None):
    """the u64 entries of the reads, record k of the stream being read perm[k] (None: as they stand); strictly ascending"""
    if perm is not None:
        p = np.asarray(perm, dtype=np.int64)
        bases, quals, lens = bases[p], (None if quals is None else quals[p]), (None if lens is None else np.asarray(lens)[p])
    m = exception_mask(bases, quals, offset, values, lens)
    rec, pos = np.nonzero(m)
    q = mapped(quals, values)[rec, pos].astype(np.uint64) & np.uint64(255) if quals is not None else np.zeros(len(rec), dtype=np.uint64)
    return bases[rec, pos].astype(np.uint64) | (q << np.uint64(8)) | (pos.astype(np.uint64) << np.uint64(16)) | (rec.astype(np.uint64) << np.uint64(28))


def records_with_one(bases, quals=None, offset=33, values=IDENTITY, lens=None):
    return int(exception_mask(bases, quals, offset, values, lens).any(axis=1).sum())


def pack(ents, read_len, nrecords):
    """the bytes of a .scalcex stream as the header documents them: the 8 magic bytes, int32 8, int32 L, int64 N, int64 X, X x u64"""
    e = np.asarray(ents, dtype="<u8")
    return b"scalce22" + struct.pack("<i", 8) + struct.pack("<i", read_len) + struct.pack("<q", nrecords) + struct.pack("<q", len(e)) + e.tobytes()


def apply(letters, quals, ents, first=0):
    """the entries put back into n x L arrays of letters and quality characters (copies); quals may be None"""
    letters = letters.copy()
    quals = None if quals is None else quals.copy()
    e = np.asarray(ents, dtype=np.uint64)
    rec = (e >> np.uint64(28)).astype(np.int64) - first
    pos = ((e >> np.uint64(16)) & np.uint64(0xFFF)).astype(np.int64)
    assert len(e) == 0 or (rec.min() >= 0 and rec.max() < letters.shape[0] and pos.max() < letters.shape[1])
    letters[rec, pos] = (e & np.uint64(255)).astype(np.uint8)
    if quals is not None:
        quals[rec, pos] = ((e >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)
    return letters, quals


def apply_text(records, ents, read_len, has_qualities, first=0, stride=1, which=0):
    """the same on records of text ("@name\\n" bases ["\\n+\\n" qualities] "\\n"): entry of record k goes to records[stride * (k - first) + which]"""
    out = [bytearray(r) for r in records]
    L = read_len
    for e in np.asarray(ents, dtype=np.uint64).tolist():
        r = out[stride * ((e >> 28) - first) + which]
        pos = (e >> 16) & 0xFFF
        assert pos < L
        last = len(r) - 1 - L
        if has_qualities:
            r[last - L - 3 + pos] = e & 255
            r[last + pos] = (e >> 8) & 255
        else:
            r[last + pos] = e & 255
    return [bytes(r) for r in out]
