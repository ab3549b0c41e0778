"""Host-side final writer: wraps the device streams of a Batch into .scalce{n,r,q} files.

Layout follows combine_and_compress_with_split (/root/reference/compress.cpp:263-343): every file
starts with the magic "scalce22"; .scalcer adds int32 no_ac and int32 read length; .scalceq adds
int64 phred offset (mate 1's for both mates) and, unless -A, the 512000 x u32 table and the u64
symbol count; .scalcen adds the names flag byte and, under -n, int64 0 plus the library name.

A variable-length run (params.variable_length) has a fourth file per mate, ours alone: .scalcel = magic, int32 entry width
(1 if L <= 255, else 2), int32 L, then one little-endian entry per record in archive order holding L - length.  The other
three files are those of the same reads padded with N to L.

A run that keeps the '+' lines (--keep-plus) has a .scalcep per mate, ours alone: magic, int32 0 (text entries), int32 P (the
longest stored entry in bytes), int64 N, then N entries in archive order, each followed by a newline.  An entry is empty (a
bare '+'), b"=" (the line repeats the header line behind its '@') or b"'" followed by the line's bytes behind the '+'.
P = 0: no entries follow, every line was bare.

A run that records what it read (--lossless --digest) has ONE .scalced, ours alone: magic, int32 16 (entry width), int32 kind
(0 one text, 1 paired files, 2 interleaved; + 4 for two-line records), int64 T (texts: 1 or 2), then T entries of {u64 bytes,
u32 crc32, u32 0}: zlib's CRC-32 of each mate stream's text as the run read it.
"""
import gzip
import struct

import numpy as np

from . import host

MAGIC = b"scalce22"


def write_archive(prefix, batch, phred_offset, library=None, gz=False):
    """Write PREFIX_<m>.scalce{n,r,q} for the shard held by `batch` (already compressed + finished)."""
    p = batch.params
    nm = 2 if p.paired else 1
    n = batch.n_reads
    opener = (lambda path: gzip.open(path, "wb", compresslevel=6)) if gz else (lambda path: open(path, "wb"))
    names = batch.output(host.OUT_NAMES, 0).tobytes() if p.use_names else b""
    for m in range(nm):
        L = p.read_len[m]
        with opener(f"{prefix}_{m + 1}.scalcer") as f:
            f.write(MAGIC + struct.pack("<ii", p.no_ac, L))
            f.write(batch.output(host.OUT_READS, m).tobytes())
        qopen = opener if p.no_ac else (lambda path: open(path, "wb"))  # AC output is never containerised (:249)
        with qopen(f"{prefix}_{m + 1}.scalceq") as f:
            f.write(MAGIC + struct.pack("<q", phred_offset))
            if not p.no_ac:
                f.write(batch.output(host.OUT_TABLE, m).tobytes())
                f.write(struct.pack("<Q", n * L))
            f.write(batch.output(host.OUT_QUAL, m).tobytes())
        with opener(f"{prefix}_{m + 1}.scalcen") as f:
            f.write(MAGIC + struct.pack("<B", 1 if p.use_names else 0))
            if p.use_names:
                f.write(names)  # mate 2's file repeats mate 1's names (compress.cpp:450-454)
            else:
                f.write(struct.pack("<q", 0) + (library or "").encode())
        if p.variable_length:
            with opener(f"{prefix}_{m + 1}.scalcel") as f:
                f.write(pack_lengths(L, batch.output(host.OUT_LENGTHS, m, np.uint16)))


def _side_header(width, param, *counts):
    """The header our side files share: magic, int32 entry width, int32 a parameter of the stream's own, then its int64 counts."""
    return MAGIC + struct.pack("<ii%dq" % len(counts), width, param, *counts)


def _side_fields(data, counts, truncated, not_ours):
    """(width, param, *counts) of a side stream's header; ValueError with `truncated` or `not_ours`, the stream's own words."""
    size = 16 + 8 * counts
    if len(data) < size:
        raise ValueError(truncated)
    if data[:7] != MAGIC[:7]:
        raise ValueError(not_ours)
    return struct.unpack("<ii%dq" % counts, data[8:size])


def length_entry_width(read_len):
    """Bytes per entry of a .scalcel stream for reads of up to read_len bases."""
    return 1 if read_len <= 255 else 2


def pack_lengths(read_len, pad):
    """The bytes of a .scalcel stream: header, then read_len - length per record (`pad`, archive order)."""
    pad = np.asarray(pad, dtype=np.int64)
    if pad.size and (pad.min() < 0 or pad.max() > read_len):
        raise ValueError("an entry of a length stream lies in 0 .. read length")
    width = length_entry_width(read_len)
    return _side_header(width, read_len) + pad.astype("<u1" if width == 1 else "<u2").tobytes()


def unpack_lengths(data):
    """(read_len, read_len - length per record) of the bytes of a .scalcel stream (out of its container)."""
    width, read_len = _side_fields(data, 0, "truncated length stream", "not a scalce length stream")
    if read_len <= 0 or read_len > 65535 or width != length_entry_width(read_len):
        raise ValueError("length stream: entry width does not fit its read length")
    if (len(data) - 16) % width:
        raise ValueError("truncated length stream")
    pad = np.frombuffer(data, dtype="<u1" if width == 1 else "<u2", offset=16).astype(np.int64)
    if pad.size and pad.max() > read_len:
        raise ValueError("length stream: an entry above the read length")
    return read_len, pad


PLUS_HEADER_BYTES = 24
PLUS_MAX_ENTRY = 65535


def pack_plus(entries):
    """The bytes of a .scalcep stream: header, then every entry followed by a newline -- or the header alone when all are empty."""
    entries = [bytes(e) for e in entries]
    for e in entries:
        if b"\n" in e:
            raise ValueError("an entry of a plus-line stream holds no newline")
        if len(e) > PLUS_MAX_ENTRY:
            raise ValueError("an entry of a plus-line stream is at most 65535 bytes long")
        if e and e != b"=" and not (e[:1] == b"'" and len(e) > 1):
            raise ValueError("plus-line stream: malformed entry")
    longest = max((len(e) for e in entries), default=0)
    return _side_header(0, longest, len(entries)) + (b"".join(e + b"\n" for e in entries) if longest else b"")


def unpack_plus(data):
    """The entries of the bytes of a .scalcep stream (out of its container); ValueError with the library's message."""
    data = bytes(data)
    width, longest, n = _side_fields(data, 1, "truncated plus-line stream", "is not a scalce plus-line stream")
    if width != 0 or longest < 0 or longest > PLUS_MAX_ENTRY or n < 0 or n > 0xFFFFFFFF:
        raise ValueError("is not a scalce plus-line stream")
    if longest == 0:
        return [b""] * n
    entries = data[PLUS_HEADER_BYTES:].split(b"\n")
    if entries.pop() != b"" or len(entries) < n:  # (the stream ends inside an entry, or before N entries)
        raise ValueError("truncated plus-line stream")
    if len(entries) != n:
        raise ValueError(f"plus-line stream holds {len(entries)} entries, its header says {n}")
    if any(len(e) > longest for e in entries):
        raise ValueError("plus-line stream: an entry is longer than its header says")
    if any(e and e != b"=" and not (e[:1] == b"'" and len(e) > 1) for e in entries):
        raise ValueError("plus-line stream: malformed entry")
    return entries


DIGEST_HEADER_BYTES = 24
DIGEST_ENTRY_WIDTH = 16


def pack_digest(kind, texts):
    """The bytes of a .scalced stream: texts = [(bytes, crc32)] of one or two texts."""
    if len(texts) not in (1, 2) or not 0 <= kind <= 6 or kind & 3 == 3:
        raise ValueError("a digest stream holds one or two texts of kind 0, 1, 2 (+ 4)")
    return _side_header(DIGEST_ENTRY_WIDTH, kind, len(texts)) + b"".join(struct.pack("<QII", n, crc, 0) for n, crc in texts)


def unpack_digest(data):
    """(kind, [(bytes, crc32)]) of the bytes of a .scalced stream (out of its container); ValueError with the library's message."""
    data = bytes(data)
    width, kind, t = _side_fields(data, 1, "truncated digest stream", "is not a scalce digest stream")
    if width != DIGEST_ENTRY_WIDTH or not 0 <= kind <= 6 or kind & 3 == 3 or t not in (1, 2):
        raise ValueError("is not a scalce digest stream")
    if len(data) < DIGEST_HEADER_BYTES + DIGEST_ENTRY_WIDTH * t:
        raise ValueError("truncated digest stream")
    if len(data) > DIGEST_HEADER_BYTES + DIGEST_ENTRY_WIDTH * t:
        raise ValueError("is not a scalce digest stream")
    out = []
    for i in range(t):
        n, crc, zero = struct.unpack_from("<QII", data, DIGEST_HEADER_BYTES + DIGEST_ENTRY_WIDTH * i)
        if zero:
            raise ValueError("is not a scalce digest stream")
        out.append((n, crc))
    return kind, out


def sample_qmap(fastq_bytes, sample=100000, lossy=0):
    """Sampling half of quality_mapping_init (qualities.cpp:64-97): first `sample` records."""
    stat = np.zeros(128, dtype=np.int64)
    pos, L = 0, 0
    data = fastq_bytes
    for _ in range(sample):
        e = pos
        for _k in range(3):
            e = data.find(b"\n", e) + 1
            if e == 0:
                break
        if e == 0:
            break
        q_end = data.find(b"\n", e)
        if q_end < 0:
            break
        q = np.frombuffer(data, dtype=np.uint8, count=q_end - e, offset=e)
        stat += np.bincount(q & 127, minlength=128)
        L = q_end - e
        pos = q_end + 1
    off, vals = host.qmap_init(stat, lossy)
    return off, vals, L
