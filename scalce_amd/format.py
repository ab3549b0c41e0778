"""Host-side final writer: wraps the device streams of a Batch into .scalce{n,r,q} files.

Layout follows combine_and_compress_with_split (/root/reference/compress.cpp:263-343): every file
starts with the magic "scalce22"; .scalcer adds int32 no_ac and int32 read length; .scalceq adds
int64 phred offset (mate 1's for both mates) and, unless -A, the 512000 x u32 table and the u64
symbol count; .scalcen adds the names flag byte and, under -n, int64 0 plus the library name.

A variable-length run (params.variable_length) has a fourth file per mate, ours alone: .scalcel = magic, int32 entry width
(1 if L <= 255, else 2), int32 L, then one little-endian entry per record in archive order holding L - length.  The other
three files are those of the same reads padded with N to L.
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


def length_entry_width(read_len):
    """Bytes per entry of a .scalcel stream for reads of up to read_len bases."""
    return 1 if read_len <= 255 else 2


def pack_lengths(read_len, pad):
    """The bytes of a .scalcel stream: header, then read_len - length per record (`pad`, archive order)."""
    pad = np.asarray(pad, dtype=np.int64)
    if pad.size and (pad.min() < 0 or pad.max() > read_len):
        raise ValueError("an entry of a length stream lies in 0 .. read length")
    width = length_entry_width(read_len)
    return MAGIC + struct.pack("<ii", width, read_len) + pad.astype("<u1" if width == 1 else "<u2").tobytes()


def unpack_lengths(data):
    """(read_len, read_len - length per record) of the bytes of a .scalcel stream (out of its container)."""
    if len(data) < 16:
        raise ValueError("truncated length stream")
    if data[:7] != MAGIC[:7]:
        raise ValueError("not a scalce length stream")
    width, read_len = struct.unpack("<ii", data[8:16])
    if read_len <= 0 or read_len > 65535 or width != length_entry_width(read_len):
        raise ValueError("length stream: entry width does not fit its read length")
    if (len(data) - 16) % width:
        raise ValueError("truncated length stream")
    pad = np.frombuffer(data, dtype="<u1" if width == 1 else "<u2", offset=16).astype(np.int64)
    if pad.size and pad.max() > read_len:
        raise ValueError("length stream: an entry above the read length")
    return read_len, pad


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
