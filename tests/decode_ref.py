"""A plain reference of the decompress path, for the tests of the decoder and the records kernel: Python and numpy, no GPU and
nothing of the product.  The rotation and the 2-bit packing of a record are the oracle's (O.pack_read), the coded frames are the
oracle's (O.AcStat.encode_stream); the text is built by string concatenation.  tests/test_decode_ref_cpu.py pins all of it
to the oracle's own archive and text before any kernel is compared with it."""
import struct

import numpy as np

import oraclelib as O

FRAME = 10 * 1024 * 1024
ROOT_CORE = 0x3FFFFFFF
MAGIC = b"scalce22"
TABLE_WORDS = 512000


def sz_read(n):
    return (n + 3) // 4


def sz_meta(L, has_buckets=True):
    return (2 if L > 255 else 1) if has_buckets else 0


# ---- records -------------------------------------------------------------------------------------------------------------
def pack_records(reads, cores, ends, L, has_buckets, lead_header=False):
    """A slice of the read stream and its directory.  reads: ASCII reads in archive order; cores: per bucket
    (core id, core string -- empty for the root bucket --, records[, the count its header states]); ends: per read, where its
    core ends (0 in the root bucket).  Headers are inline in front of every bucket but the first (lead_header: of that too, as
    the whole stream has it).  has_buckets = 0: bare records of mate 2, one directory entry.
    Returns (bytes, [dict(first, off, core_len, rec_bytes, core)])."""
    out = bytearray()
    if not has_buckets:
        for r in reads:
            assert len(r) == L
            out += O.pack_read(np.frombuffer(r, dtype=np.uint8), 0, 0).tobytes()
        return bytes(out), [dict(first=0, off=0, core_len=0, rec_bytes=sz_read(L), core=b"")]
    meta = sz_meta(L)
    directory = []
    k = 0
    for bi, bucket in enumerate(cores):
        cid, core, cnt = bucket[:3]
        if bi or lead_header:
            out += struct.pack("<iQ", cid, bucket[3] if len(bucket) > 3 else cnt)
        if not cnt:
            continue
        directory.append(dict(first=k, off=len(out), core_len=len(core), rec_bytes=sz_read(L - len(core)) + meta, core=core))
        for r, e in zip(reads[k:k + cnt], ends[k:k + cnt]):
            assert len(r) == L and (e == 0) == (len(core) == 0) and (not e or r[e - len(core):e] == core), (r, core, e)
            n, l = (e - len(core), len(core)) if e else (0, 0)
            out += O.pack_read(np.frombuffer(r, dtype=np.uint8), n, l).tobytes() + int(e).to_bytes(meta, "little")
        k += cnt
    assert k == len(reads) == len(ends)
    return bytes(out), directory


def window_records(reads, cores, ends, L, has_buckets, a, b):
    """pack_records of records [a, b): the directory window-relative, the first bucket's header outside the slice, the headers of
    the buckets that begin inside it inline, each stating its bucket's whole count"""
    if not has_buckets:
        return pack_records(reads[a:b], None, None, L, 0)
    cut, s = [], 0
    for cid, core, cnt in cores:
        lo, hi = max(a, s), min(b, s + cnt)
        if hi > lo:
            cut.append((cid, core, hi - lo, cnt))
        s += cnt
    return pack_records(reads[a:b], cut, ends[a:b], L, 1)


def unpack_records(payload, L, core_of, has_buckets=True, nrecords=None):
    """The inverse, for a whole read stream behind its 16-byte header: (reads, cores, ends) as pack_records takes them.
    core_of(id) -> core string."""
    reads, cores, ends = [], [], []

    def bases(rec, n):
        return bytes(b"ACGT"[(rec[i >> 2] >> ((~i & 3) << 1)) & 3] for i in range(n))
    if not has_buckets:
        rb = sz_read(L)
        assert len(payload) == nrecords * rb
        return [bases(payload[k * rb:(k + 1) * rb], L) for k in range(nrecords)], None, None
    meta = sz_meta(L)
    pos = 0
    while pos < len(payload):
        cid, cnt = struct.unpack_from("<iQ", payload, pos)
        pos += 12
        core = b"" if cid == ROOT_CORE else core_of(cid)
        cores.append((cid, core, cnt))
        nb = sz_read(L - len(core))
        for _ in range(cnt):
            e = int.from_bytes(payload[pos + nb:pos + nb + meta], "little")
            stored = bases(payload[pos:pos + nb], L - len(core))  # behind the core, then in front of it
            reads.append(stored[L - e:] + core + stored[:L - e] if e else stored)
            ends.append(e)
            pos += nb + meta
    assert pos == len(payload)
    return reads, cores, ends


def pack_root_records(bases2d):
    """pack_records of ACGT reads that all lie in the root bucket (end 0, read length a multiple of 4, at most 255), vectorised:
    the records without a header"""
    n, L = bases2d.shape
    assert L % 4 == 0 and L <= 255
    lut = np.zeros(256, dtype=np.uint8)
    lut[[ord(c) for c in "ACGT"]] = (0, 1, 2, 3)
    c = lut[bases2d].reshape(n, L // 4, 4)
    rec = np.zeros((n, L // 4 + 1), dtype=np.uint8)
    rec[:, :-1] = (c[:, :, 0] << 6) | (c[:, :, 1] << 4) | (c[:, :, 2] << 2) | c[:, :, 3]
    return rec.tobytes()


# ---- names ----------------------------------------------------------------------------------------------------------------
def pack_names(names):
    """[u8 n][n bytes] per name, and where each starts (len + 1 entries)"""
    out, off = bytearray(), []
    for nm in names:
        off.append(len(out))
        out += bytes([len(nm)]) + nm
    return bytes(out), off + [len(out)]


def unpack_names(payload, nrecords):
    names, pos = [], 0
    for _ in range(nrecords):
        names.append(payload[pos + 1:pos + 1 + payload[pos]])
        pos += 1 + payload[pos]
    assert pos == len(payload)
    return names


# ---- text -----------------------------------------------------------------------------------------------------------------
def record_texts(reads, quals, names, phred, mate_digit):
    """one string per record.  quals: rows of quality symbols, or None for two-line records; names: the stored names, or
    (library, first) for "<library>.<first + k>"; mate_digit: 0, or the character a trailing "/x" gets (stored names only)"""
    recs = []
    for k, r in enumerate(reads):
        if isinstance(names, tuple):
            nm = names[0] + b"." + str(names[1] + k).encode()
        else:
            nm = names[k]
            if mate_digit and len(nm) > 1 and nm[-2:-1] == b"/":
                nm = nm[:-1] + bytes([mate_digit])
        if quals is None:
            recs.append(b"@" + nm + b"\n" + r + b"\n")
        else:
            q = bytes(quals[k])
            assert len(q) == len(r)
            line = bytes(ord("N") if s == 0 else c for c, s in zip(r, q))
            recs.append(b"@" + nm + b"\n" + line + b"\n+\n" + bytes((s + phred) & 0xFF for s in q) + b"\n")
    return recs


def text_of(reads, quals, names, phred, mate_digit, interleave=None):
    """The FASTQ (quals given) or two-line text of the records, and where each record starts in it with the text's end
    appended.  interleave: (reads, quals, names, phred, mate_digit) of mate 2 -- the text then holds mate 1 and mate 2 of
    each pair one after the other, and the offsets are the pairs'."""
    recs = record_texts(reads, quals, names, phred, mate_digit)
    if interleave is not None:
        other = record_texts(*interleave)
        assert len(other) == len(recs)
        recs = [x + y for x, y in zip(recs, other)]
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    return b"".join(recs), offs


def text_of_uniform(bases2d, quals2d, library, first, phred):
    """text_of(reads, quals, (library, first), phred, 0)[0] for hundreds of thousands of records: the records whose index has
    the same number of digits form one matrix of bytes"""
    n, L = bases2d.shape
    line = np.where(quals2d == 0, np.uint8(ord("N")), bases2d)
    ql = (quals2d.astype(np.uint32) + phred).astype(np.uint8)
    head = np.frombuffer(b"@" + library + b".", dtype=np.uint8)
    parts = []
    k = 0
    while k < n:
        d = len(str(first + k))
        hi = min(n, 10 ** d - first)
        idx = np.arange(first + k, first + hi, dtype=np.uint64)
        m = np.empty((hi - k, len(head) + d + 1 + L + 3 + L + 1), dtype=np.uint8)
        m[:, :len(head)] = head
        for j in range(d):
            m[:, len(head) + j] = (idx // np.uint64(10 ** (d - 1 - j))) % np.uint64(10) + np.uint64(48)
        c = len(head) + d
        m[:, c] = 10
        m[:, c + 1:c + 1 + L] = line[k:hi]
        m[:, c + 1 + L:c + 4 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
        m[:, c + 4 + L:c + 4 + 2 * L] = ql[k:hi]
        m[:, c + 4 + 2 * L] = 10
        parts.append(m.tobytes())
        k = hi
    return b"".join(parts)


# ---- the quality stream ---------------------------------------------------------------------------------------------------
def framed(table, sym):
    """the oracle's coded frames of a symbol stream, [u32 size][bytes] per 10 485 760 symbols -- never the GPU encoder's"""
    return O.AcStat(table).encode_stream(sym).tobytes()


def frames_of(coded, nframes):
    """[(offset of the size word, size)] of the first `nframes` frames"""
    out, pos = [], 0
    for _ in range(nframes):
        sz = struct.unpack_from("<I", coded, pos)[0]
        out.append((pos, sz))
        pos += 4 + sz
    assert pos <= len(coded)
    return out


# ---- archive files --------------------------------------------------------------------------------------------------------
def read_stream_file(L, payload, no_ac=0):
    return MAGIC + struct.pack("<ii", no_ac, L) + payload


def name_stream_file(names_payload=None, library=None):
    if names_payload is not None:
        return MAGIC + b"\x01" + names_payload
    return MAGIC + b"\x00" + struct.pack("<q", 0) + library


def quality_stream_file(phred, table, nsym, coded):
    return MAGIC + struct.pack("<q", phred) + np.ascontiguousarray(table, dtype=np.uint32).tobytes() + struct.pack("<Q", nsym) + coded


def parse_archive(r, n, q, paired_names=False):
    """The three files of one mate as the oracle wrote them (no -A): dict(L, payload, names or None, library, phred, table,
    nsym, coded)"""
    assert r[:8] == MAGIC and n[:8] == MAGIC and q[:8] == MAGIC
    no_ac, L = struct.unpack_from("<ii", r, 8)
    assert no_ac == 0
    phred = struct.unpack_from("<q", q, 8)[0]
    table = np.frombuffer(q, dtype=np.uint32, count=TABLE_WORDS, offset=16)
    nsym = struct.unpack_from("<Q", q, 16 + 4 * TABLE_WORDS)[0]
    out = dict(L=L, payload=r[16:], phred=phred, table=table, nsym=nsym, coded=q[24 + 4 * TABLE_WORDS:], names=None, library=None)
    if n[8]:
        out["names"] = n[9:]
    else:
        out["library"] = n[17:]
    return out


def decode_symbols(table, coded, nsym):
    """the oracle's decoder over the frames"""
    st = O.AcStat(table)
    nfr = (nsym + FRAME - 1) // FRAME
    parts = []
    for i, (pos, sz) in enumerate(frames_of(coded, nfr)):
        parts.append(st.decode_block(np.frombuffer(coded, dtype=np.uint8, count=sz, offset=pos + 4), min(FRAME, nsym - i * FRAME)))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
