"""ctypes host over include/scalce_hip.h.

Names follow the reference's seam: a Context carries the core table
(read_patterns / prepare_aho_automata), a Batch is one FASTQ shard resident in HBM, and its stage
methods are the batched forms of aho_search / output_read / output_quality / aho_trie_bucket /
aho_output / set_ac_stat / ac_write.  PyTorch is only used by callers for device memory; this
module takes raw device pointers.
"""
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

OUT_READS, OUT_NAMES, OUT_QUAL, OUT_TABLE, OUT_FREQ4, OUT_TOKENS, OUT_PERM, OUT_QSTREAM, OUT_BUCKET_COUNTS, OUT_QINPUT, OUT_NAMELEN = range(11)
OUT_LENGTHS = 12  # variable-length runs: N x u16, read_len - length per record in output order
OUT_NAMECELLS = 13  # for tests: N x 16 bytes, [stored length][first 15 characters, zero behind a shorter name], input order
OUT_COMMENTS = 14  # keep_comments: what follows the name of every record in output order, each entry followed by a newline
OUT_PLUS = 16  # keep_plus: the '+'-line entry of every record in output order, each followed by a newline
OUT_EXCEPTIONS = 15  # keep_bases: u64 entries in output order: letter | values[q] << 8 | position << 16 | record << 28
STAGES = ("ingest", "quality", "tokenize", "order", "emit", "entropy")
ROOT_CORE = 0x3FFFFFFF


class ScalceError(RuntimeError):
    pass


def library_path():
    return os.path.join(_HERE, "lib", "libscalce_hip.so")


class QMap(C.Structure):
    _fields_ = [("offset", C.c_int32), ("values", C.c_int32 * 128)]


class Params(C.Structure):
    _fields_ = [("read_len", C.c_int32 * 2), ("paired", C.c_int32), ("use_names", C.c_int32), ("no_ac", C.c_int32),
                ("qmap", QMap * 2), ("bucket_set_size", C.c_uint64), ("qprev", (C.c_uint32 * 2) * 2),
                ("fasta", C.c_int32), ("no_qualities", C.c_int32), ("interleaved", C.c_int32), ("variable_length", C.c_int32)]


class ShardResult(C.Structure):
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("nb1", C.c_uint32), ("rounds", C.c_uint32), ("sweeps", C.c_uint32),
                ("chunks_total", C.c_uint32), ("reads_total", C.c_uint64), ("first_read", C.c_uint64), ("reads_local", C.c_uint64),
                ("moved_in", C.c_uint64 * 2), ("counts", C.POINTER(C.c_uint64)), ("name_bytes", C.POINTER(C.c_uint64)),
                ("sym_lo", C.c_uint64 * 2), ("sym_hi", C.c_uint64 * 2), ("coded_bytes", (C.c_uint64 * 64) * 2),
                ("keep", C.c_void_p * 8), ("keep_bytes", C.c_uint64 * 8), ("magic", C.c_uint32)]


class FqBucket(C.Structure):
    """scalce_fq_bucket: one bucket of a window's directory (host_decode.inc asserts the layout against the kernel's)"""
    _fields_ = [("first", C.c_uint64), ("off", C.c_uint64), ("core_len", C.c_uint32), ("rec_bytes", C.c_uint32),
                ("core", C.c_char * 32)]


class FqWindow(C.Structure):
    """scalce_fq_window: every pointer is the caller's device memory (library: host)"""
    _fields_ = [("d_reads", C.c_void_p), ("d_dir", C.c_void_p), ("nbuckets", C.c_uint32), ("read_len", C.c_int32),
                ("has_buckets", C.c_int32), ("mate_digit", C.c_int32), ("nrecords", C.c_uint64), ("first_record", C.c_uint64),
                ("d_qual", C.c_void_p), ("phred_offset", C.c_int64), ("d_names", C.c_void_p), ("d_name_off", C.c_void_p),
                ("library", C.c_char_p), ("d_out", C.c_void_p), ("d_record_offsets", C.c_void_p), ("interleave", C.c_int32),
                ("pair_read_len", C.c_int32), ("d_pair_name_off", C.c_void_p)]


SHARD_PREPARE_ONLY, SHARD_CODER_ASYNC = 1, 2
APPEND_FINAL, APPEND_NO_QUALITY, APPEND_NO_TOKENIZE = 1, 2, 4  # SCALCE_APPEND_*
# scalce_patterns_walk / scalce_patterns_walk_host, by SCALCE_WALK_* value
WALKS = ("none", "kmer", "kmer_t7", "anchor")


def lib():
    """Load the HIP library; fail loudly when it has not been built (no fallback exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ScalceError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). scalce_amd has no CPU implementation.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64; if the
    # system copy gets loaded first (through this library's NEEDED entry) torch later finds no GPU.  Loading
    # torch first makes the dynamic linker resolve our libamdhip64.so.7 to the copy torch already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.scalce_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.scalce_ctx_destroy.argtypes = [vp]
    L.scalce_last_error.argtypes = [vp]
    L.scalce_last_error.restype = C.c_char_p
    L.scalce_patterns_load_bin.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.scalce_patterns_load_text.argtypes = [vp, C.c_char_p, C.c_size_t]
    for f in ("scalce_patterns_count", "scalce_patterns_states", "scalce_patterns_buckets"):
        getattr(L, f).argtypes = [vp]
    L.scalce_patterns_walk.argtypes = [vp, C.POINTER(C.c_int)]
    L.scalce_pattern_length.argtypes = [vp, i32]
    L.scalce_pattern_string.argtypes = [vp, i32]
    L.scalce_pattern_string.restype = C.c_char_p
    L.scalce_qmap_init.argtypes = [C.POINTER(QMap), C.POINTER(C.c_int32), i32]
    L.scalce_qmap_init.restype = None
    L.scalce_params_default.argtypes = [C.POINTER(Params)]
    L.scalce_params_default.restype = None
    L.scalce_batch_create.argtypes = [vp, C.POINTER(Params), u64, u64, C.POINTER(vp)]
    L.scalce_batch_destroy.argtypes = [vp]
    L.scalce_workspace_create.argtypes = [vp, C.POINTER(vp)]
    L.scalce_workspace_destroy.argtypes = [vp]
    L.scalce_workspace_destroy.restype = None
    L.scalce_batch_create_shared.argtypes = [vp, C.POINTER(Params), u64, u64, vp, C.POINTER(vp)]
    L.scalce_batch_ingest.argtypes = [vp, i32, vp, u64, vp]
    L.scalce_batch_append.argtypes = [vp, vp, u64, vp, u64, i32, C.POINTER(u64), vp]
    L.scalce_batch_reset.argtypes = [vp]
    L.scalce_batch_set_lean.argtypes = [vp, i32]
    L.scalce_batch_set_lean.restype = None
    L.scalce_batch_quality.argtypes = [vp, vp]
    L.scalce_batch_quality_plan.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    L.scalce_batch_ingest_plan.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    L.scalce_batch_tokenize.argtypes = [vp, vp, vp]
    L.scalce_batch_order.argtypes = [vp, vp]
    L.scalce_batch_emit.argtypes = [vp, vp]
    L.scalce_batch_entropy.argtypes = [vp, vp, vp]
    L.scalce_batch_entropy_begin.argtypes = [vp, vp, vp]
    L.scalce_batch_entropy_end.argtypes = [vp, vp]
    L.scalce_batch_entropy_stream_begin.argtypes = [vp, i32, vp, vp, u64, vp]
    L.scalce_batch_entropy_stream_prepare.argtypes = [vp, i32, vp, vp, u64, vp]
    L.scalce_batch_entropy_begin_group.argtypes = [C.POINTER(vp), i32, vp, vp]
    L.scalce_batch_entropy_begin_group_last.argtypes = [C.POINTER(vp), i32, vp, vp, i32]
    L.scalce_batch_compress.argtypes = [vp, vp, u64, vp, u64, vp]
    L.scalce_batch_front.argtypes = [vp, vp, u64, vp, u64, vp]
    L.scalce_batch_finish.argtypes = [vp, vp]
    L.scalce_batch_output.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(u64)]
    L.scalce_batch_set_frame_on_demand.argtypes = [vp, i32]
    L.scalce_batch_qual_bytes.argtypes = [vp, i32, C.POINTER(u64)]
    L.scalce_batch_qual_window.argtypes = [vp, i32, u64, u64, vp, vp]
    L.scalce_batch_reads.argtypes = [vp]
    L.scalce_batch_reads.restype = u64
    L.scalce_batch_stage_ms.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(i32)]
    L.scalce_batch_stage_reset.argtypes = [vp, i32]
    L.scalce_batch_stage_reset.restype = None
    L.scalce_batch_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.scalce_batch_tie_plan.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.scalce_batch_kernel_timing.argtypes = [vp, i32]
    L.scalce_batch_kernel_timing.restype = None
    L.scalce_batch_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(u64), C.POINTER(u64)]
    L.scalce_memcpy_d2h.argtypes = [vp, vp, vp, u64]
    L.scalce_memcpy_h2d.argtypes = [vp, vp, vp, u64]
    L.scalce_memcpy_d2d.argtypes = [vp, vp, vp, u64, vp]
    L.scalce_batch_tokenize_begin.argtypes = [vp, vp]
    L.scalce_batch_tokenize_end.argtypes = [vp, vp]
    L.scalce_batch_tokenize_settle.argtypes = [vp, vp, vp]
    L.scalce_batch_set_chunks.argtypes = [vp, C.POINTER(u64), C.c_uint32]
    L.scalce_batch_entropy_stream.argtypes = [vp, i32, vp, vp, u64, vp]
    L.scalce_ac_scale.argtypes = [vp, vp, C.c_uint32, vp, vp]
    L.scalce_batch_chunk_plan.argtypes = [vp, u64, C.POINTER(u64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(u64), vp]
    L.scalce_batch_text_offset.argtypes = [vp, i32, u64, C.POINTER(u64), vp]
    L.scalce_batch_rewindow.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), vp]
    L.scalce_batch_qinput_edges.argtypes = [vp, i32, C.POINTER(C.c_uint8), C.POINTER(u64), C.POINTER(C.c_int32), vp]
    L.scalce_batch_set_fused_rows.argtypes = [vp, i32]
    L.scalce_comm_unique_id.argtypes = [C.c_char_p]
    L.scalce_comm_create_rccl.argtypes = [i32, i32, i32, C.c_char_p, C.POINTER(vp)]
    L.scalce_comm_create_shm.argtypes = [i32, i32, i32, C.c_char_p, u64, C.POINTER(vp)]
    L.scalce_comm_destroy.argtypes = [vp]
    L.scalce_comm_error.argtypes = [vp]
    L.scalce_comm_error.restype = C.c_char_p
    L.scalce_comm_barrier.argtypes = [vp, vp]
    L.scalce_comm_all_gather.argtypes = [vp, vp, vp, u64, vp]
    L.scalce_comm_all_reduce_sum_u64.argtypes = [vp, vp, u64, vp]
    L.scalce_comm_all_to_all_v.argtypes = [vp, vp, C.POINTER(u64), vp, C.POINTER(u64), vp]
    L.scalce_sharded_compress.argtypes = [vp, vp, vp, vp, u64, vp, u64, i32, vp, vp, C.POINTER(ShardResult)]
    L.scalce_shard_result_free.argtypes = [C.POINTER(ShardResult)]
    L.scalce_shard_result_free.restype = None
    L.scalce_copy_pieces.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, u64, vp]
    L.scalce_patterns_describe_host.argtypes = [C.c_char_p, C.c_size_t, i32, vp, C.c_size_t, C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32)]
    L.scalce_patterns_walk_host.argtypes = [C.c_char_p, C.c_size_t, i32, C.POINTER(C.c_int)]
    L.scalce_selftest_ac.argtypes = [vp, u64, C.c_uint32, i32, C.POINTER(C.c_uint32)]
    L.scalce_ac_decode.argtypes = [vp, vp, vp, u64, u64, vp, vp]
    L.scalce_fastq_text_bytes.restype = u64
    L.scalce_fastq_text_bytes.argtypes = [i32, u64, u64, C.c_char_p]
    L.scalce_fasta_text_bytes.restype = u64
    L.scalce_fasta_text_bytes.argtypes = [i32, u64, u64, C.c_char_p]
    L.scalce_fastq_records.argtypes = [vp, i32, i32, vp, u64, u64, vp, C.c_int64, vp, u64, C.c_char_p, i32, vp, u64,
                                       C.POINTER(u64), vp, vp]
    L.scalce_ac_decoder_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.scalce_ac_decoder_destroy.argtypes = [vp]
    L.scalce_ac_decoder_destroy.restype = None
    L.scalce_ac_decoder_device_bytes.argtypes = [vp]
    L.scalce_ac_decoder_device_bytes.restype = u64
    L.scalce_ac_decoder_launch.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, vp, vp, vp, vp]
    L.scalce_fastq_records_window.argtypes = [vp, C.POINTER(FqWindow), vp]
    _LIB = L
    return L


def qmap_init(stat, lossy_percentage):
    """quality_mapping_init after sampling (qualities.cpp:99-174) -> (offset, values[128])."""
    q = QMap()
    st = (C.c_int32 * 128)(*[int(x) for x in stat[:128]])
    lib().scalce_qmap_init(C.byref(q), st, int(lossy_percentage))
    return q.offset, np.array(list(q.values), dtype=np.int32)


def walk_of_table(blob, is_text=False):
    """Context.walk of a core table without a device: (name, K); ("none", 0) for a table the loaders refuse."""
    k = C.c_int(0)
    w = lib().scalce_patterns_walk_host(blob, len(blob), int(is_text), C.byref(k))
    return WALKS[w], k.value


class Context:
    def __init__(self, device=0, patterns_bin=None, patterns_text=None):
        self.L = lib()
        self.h = C.c_void_p()
        self.device = int(device)
        self._table = (patterns_bin, 0) if patterns_bin is not None else (patterns_text, 1)
        rc = self.L.scalce_ctx_create(int(device), C.byref(self.h))
        if rc:
            msg = self.L.scalce_last_error(self.h).decode() if self.h else "scalce_ctx_create failed"
            raise ScalceError(msg)
        if patterns_bin is not None:
            self._check(self.L.scalce_patterns_load_bin(self.h, patterns_bin, len(patterns_bin)))
        elif patterns_text is not None:
            self._check(self.L.scalce_patterns_load_text(self.h, patterns_text, len(patterns_text)))

    def _check(self, rc):
        if rc:
            raise ScalceError(f"[{rc}] " + self.L.scalce_last_error(self.h).decode())

    @property
    def n_patterns(self):
        return self.L.scalce_patterns_count(self.h)

    @property
    def n_states(self):
        return self.L.scalce_patterns_states(self.h)

    @property
    def n_buckets(self):
        return self.L.scalce_patterns_buckets(self.h)

    @property
    def walk(self):
        """The tokenizer walk the loaded table selects: (name, K) with name one of WALKS; K > 0 only for "anchor"."""
        k = C.c_int(0)
        w = self.L.scalce_patterns_walk(self.h, C.byref(k))
        return WALKS[w], k.value

    def pattern(self, p):
        return self.L.scalce_pattern_string(self.h, p)

    def to_host(self, d_ptr, nbytes, dtype=np.uint8):
        out = np.empty(int(nbytes), dtype=np.uint8)
        if nbytes:
            self._check(self.L.scalce_memcpy_d2h(self.h, out.ctypes.data, d_ptr, int(nbytes)))
        return out.view(dtype)

    def selftest_ac(self, ncases=1 << 24, seed=1, general=False):
        out = (C.c_uint32 * 6)()
        self._check(self.L.scalce_selftest_ac(self.h, int(ncases), int(seed), int(general), out))
        return list(out)

    def bucket_patterns(self):
        """File-order core index of every bucket in emission order, root (0x3FFFFFFF) last."""
        blob, is_text = self._table
        out = np.zeros(self.n_buckets + 1, dtype=np.int32)
        ns, nb = C.c_int32(), C.c_int32()
        self._check(self.L.scalce_patterns_describe_host(blob, len(blob), is_text, out.ctypes.data, len(out),
                                                         C.byref(ns), C.byref(nb)))
        return out

    def copy_pieces(self, d_src, d_dst, d_piece_src, d_piece_dst, npieces, total, stream=0):
        self._check(self.L.scalce_copy_pieces(self.h, d_src, d_dst, d_piece_src, d_piece_dst, int(npieces), int(total), stream))

    def ac_scale(self, d_counters, factor, d_table, stream=0):
        """compress.cpp:297-313 on the device: table = max(1, (1 + counters) / factor)."""
        self._check(self.L.scalce_ac_scale(self.h, d_counters, int(factor), d_table, stream))

    def copy_d2d(self, dst, src, nbytes, stream=0):
        self._check(self.L.scalce_memcpy_d2d(self.h, dst, src, int(nbytes), stream))

    def fastq_records(self, read_len, reads_payload, nrecords, d_qual, phred, names_payload=None, library=None, has_buckets=True,
                      mate_digit=0, stream=0):
        """Records back to FASTQ text on the device (scalce_fastq_records); returns the text as bytes.  d_qual = None: the
        two-line records of an archive without qualities."""
        import torch
        reads = np.frombuffer(reads_payload, dtype=np.uint8)
        names = None if names_payload is None else np.frombuffer(names_payload, dtype=np.uint8)
        lib = None if library is None else library.encode()
        text_bytes = self.L.scalce_fastq_text_bytes if d_qual is not None else self.L.scalce_fasta_text_bytes
        cap = text_bytes(read_len, nrecords, 0 if names is None else len(names), None if names is not None else lib)
        out = torch.empty(cap + 64, dtype=torch.uint8, device=f"cuda:{self.device}")
        nb = C.c_uint64(0)
        self._check(self.L.scalce_fastq_records(self.h, read_len, int(has_buckets), reads.ctypes.data, len(reads), nrecords, d_qual,
                                                int(phred), None if names is None else names.ctypes.data,
                                                0 if names is None else len(names), lib or b"", mate_digit, out.data_ptr(), cap,
                                                C.byref(nb), None, stream))
        return out[: nb.value].cpu().numpy().tobytes()

    def ac_decode(self, table_u32, d_blocks, nbytes, nsym, d_out, stream=0):
        t = np.ascontiguousarray(table_u32, dtype=np.uint32)
        self._check(self.L.scalce_ac_decode(self.h, t.ctypes.data, d_blocks, int(nbytes), int(nsym), d_out, stream))

    def ac_decoder(self, table_u32, stream=0):
        """What scalce_ac_decoder_create prepares from a table, once: launch() then decodes runs of whole frames."""
        return AcDecoder(self, table_u32, stream)

    def fastq_records_window(self, d_reads, d_dir, nbuckets, read_len, nrecords, d_out, first_record=0, has_buckets=True,
                             mate_digit=0, d_qual=None, phred=33, d_names=None, d_name_off=None, library=None,
                             d_record_offsets=None, interleave=0, pair_read_len=0, d_pair_name_off=None, stream=0):
        """One window of whole records into text (scalce_fastq_records_window): enqueues the kernel on `stream`, nothing else.
        Every d_* is a device pointer of the caller's, at any byte address the entry allows; d_dir points at `nbuckets`
        FqBucket entries, window-relative; library: str or bytes, for names "<library>.<first_record + k>"."""
        if isinstance(library, str):
            library = library.encode()
        w = FqWindow(d_reads, d_dir, int(nbuckets), int(read_len), int(has_buckets), int(mate_digit), int(nrecords),
                     int(first_record), d_qual, int(phred), d_names, d_name_off, library, d_out, d_record_offsets,
                     int(interleave), int(pair_read_len), d_pair_name_off)
        self._check(self.L.scalce_fastq_records_window(self.h, C.byref(w), stream))

    def close(self):
        if self.h:
            self.L.scalce_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AcDecoder:
    """scalce_ac_decoder: the arithmetic decoder of one table (scalce_ac_decoder_create / _launch / _destroy)."""

    def __init__(self, ctx, table_u32, stream=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        t = np.ascontiguousarray(table_u32, dtype=np.uint32)
        ctx._check(ctx.L.scalce_ac_decoder_create(ctx.h, t.ctypes.data, stream, C.byref(self.h)))

    @property
    def device_bytes(self):
        return int(self.ctx.L.scalce_ac_decoder_device_bytes(self.h))

    def launch(self, d_frames, nbytes, nframes, nsym, d_out, stream=0):
        """Decodes `nframes` whole frames that begin at d_frames (nbytes of them are there) into d_out and waits for it.
        Returns the frame walk's verdict word: != 0, the bytes end before the frames do."""
        import torch
        dev = f"cuda:{self.ctx.device}"
        d_off = torch.zeros(max(1, int(nframes)), dtype=torch.int64, device=dev)
        d_size = torch.zeros(int(nframes) + 1, dtype=torch.int32, device=dev)  # the sizes and, behind them, the verdict
        d_bad = d_size.data_ptr() + 4 * int(nframes)
        self.ctx._check(self.ctx.L.scalce_ac_decoder_launch(self.h, d_frames, int(nbytes), int(nframes), int(nsym), d_off.data_ptr(),
                                                            d_size.data_ptr(), d_bad, d_out, stream))
        torch.cuda.synchronize(dev)
        return int(d_size[int(nframes)].item()) & 0xFFFFFFFF

    def close(self):
        if self.h:
            self.ctx.L.scalce_ac_decoder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """Collectives of a sharded run (scalce_comm): RCCL between processes with one GPU each, or the shared-memory
    rehearsal transport between processes that share a GPU."""

    def __init__(self, device, world, rank, unique_id=None, shm_name=None, slot_bytes=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.world, self.rank = world, rank
        if shm_name is not None:
            rc = self.L.scalce_comm_create_shm(device, world, rank, shm_name.encode(), int(slot_bytes), C.byref(self.h))
        else:
            rc = self.L.scalce_comm_create_rccl(device, world, rank, unique_id, C.byref(self.h))
        if rc:
            raise ScalceError(f"[{rc}] " + (self.L.scalce_comm_error(self.h) or b"").decode())

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        if lib().scalce_comm_unique_id(buf):
            raise ScalceError("RCCL is not available (ncclGetUniqueId)")
        return buf.raw

    def _check(self, rc):
        if rc:
            raise ScalceError(f"[{rc}] " + self.L.scalce_comm_error(self.h).decode())

    def barrier(self, stream=0):
        self._check(self.L.scalce_comm_barrier(self.h, stream))

    def all_gather(self, d_send, d_recv, nbytes, stream=0):
        self._check(self.L.scalce_comm_all_gather(self.h, d_send, d_recv, int(nbytes), stream))

    def all_reduce_sum_u64(self, d_buf, count, stream=0):
        self._check(self.L.scalce_comm_all_reduce_sum_u64(self.h, d_buf, int(count), stream))

    def all_to_all_v(self, d_send, send_bytes, d_recv, recv_bytes, stream=0):
        """send_bytes[d] bytes to every rank d (consecutive ranges of d_send), recv_bytes[src] from every rank src."""
        sb = (C.c_uint64 * self.world)(*[int(x) for x in send_bytes])
        rb = (C.c_uint64 * self.world)(*[int(x) for x in recv_bytes])
        self._check(self.L.scalce_comm_all_to_all_v(self.h, d_send, sb, d_recv, rb, stream))

    def close(self):
        if self.h:
            self.L.scalce_comm_destroy(self.h)
            self.h = C.c_void_p()


def sharded_compress(comm, ctx, batch, d_text1, n1, d_text2=None, n2=0, flags=0, stream=0, coder_stream=0, result=None):
    """SPMD body of a sharded run (scalce_sharded_compress); returns the ShardResult (free it with shard_result_free).
    `result`: the result of an earlier call on the same batch -- its device buffers are reused."""
    res = result if result is not None else ShardResult()
    rc = ctx.L.scalce_sharded_compress(comm.h, ctx.h, batch.h, d_text1, int(n1), d_text2, int(n2), int(flags), stream, coder_stream,
                                       C.byref(res))
    if rc:
        raise ScalceError(f"[{rc}] sharded run failed on rank {comm.rank}: " + ctx.L.scalce_last_error(ctx.h).decode(errors="replace"))
    return res


def shard_plan_blocks(world, rank, nb1, counts, read_len):
    """scalce_shard_plan_blocks: the run-wide reordered quality stream dealt out in ranges of whole 10 MiB blocks.
    counts = [world][nb1] reads per (rank, bucket).  Returns (send_bytes, recv_bytes, lo, hi, piece_src, piece_dst)."""
    L = lib()
    u64p = C.POINTER(C.c_uint64)
    L.scalce_shard_plan_blocks.argtypes = [C.c_int, C.c_int, C.c_uint32, u64p, C.c_uint64, u64p, u64p, u64p, u64p, u64p, u64p, u64p]
    flat = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    send, recv = np.zeros(world, np.uint64), np.zeros(world, np.uint64)
    ps, pd = np.zeros(world * nb1 + 1, np.uint64), np.zeros(world * nb1 + 1, np.uint64)
    lo, hi, npc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.scalce_shard_plan_blocks(world, rank, nb1, flat.ctypes.data_as(u64p), int(read_len), send.ctypes.data_as(u64p),
                                    recv.ctypes.data_as(u64p), C.byref(lo), C.byref(hi), ps.ctypes.data_as(u64p), pd.ctypes.data_as(u64p),
                                    C.byref(npc))
    if rc:
        raise ScalceError(f"[{rc}] scalce_shard_plan_blocks")
    return send, recv, int(lo.value), int(hi.value), ps[: npc.value].copy(), pd[: npc.value].copy()


def shard_plan_edge_trigrams(world, rank, nsym, edges):
    """scalce_shard_plan_edge_trigrams: the trigram counters that straddle the boundary in front of `rank`'s original piece.
    nsym = [world] symbols per piece, edges = [world][4] in scalce_batch_qinput_edges' layout.  Returns the list of keys."""
    L = lib()
    L.scalce_shard_plan_edge_trigrams.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_uint64,
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    ns = np.ascontiguousarray(nsym, dtype=np.uint64)
    ed = np.ascontiguousarray(edges, dtype=np.uint8).reshape(world, 4)
    keys, nk = (C.c_uint32 * 2)(), C.c_uint32()
    rc = L.scalce_shard_plan_edge_trigrams(world, rank, ns.ctypes.data_as(C.POINTER(C.c_uint64)), ed.ctypes.data_as(C.POINTER(C.c_uint8)), 4,
                                           keys, C.byref(nk))
    if rc:
        raise ScalceError(f"[{rc}] scalce_shard_plan_edge_trigrams")
    return list(keys[: nk.value])


def shard_plan_own_pieces(world, rank, send_bytes, recv_bytes, piece_src, piece_dst):
    """scalce_shard_plan_own_pieces: the pieces of shard_plan_blocks split into those that read the local stream and those
    that read the receive buffer without the own bytes.
    Returns (own_src, own_dst, own_total, local_off, other_src, other_dst, other_total)."""
    L = lib()
    u64p = C.POINTER(C.c_uint64)
    L.scalce_shard_plan_own_pieces.argtypes = [C.c_int, C.c_int, u64p, u64p, u64p, u64p, C.c_uint64] + [u64p] * 9
    ins = [np.ascontiguousarray(a, dtype=np.uint64) for a in (send_bytes, recv_bytes, piece_src, piece_dst)]
    n = len(ins[2])
    os_, od, xs, xd = (np.zeros(n + 1, np.uint64) for _ in range(4))
    no, ot, off, nx, xt = (C.c_uint64() for _ in range(5))
    rc = L.scalce_shard_plan_own_pieces(world, rank, *(a.ctypes.data_as(u64p) for a in ins), n, os_.ctypes.data_as(u64p), od.ctypes.data_as(u64p),
                                        C.byref(no), C.byref(ot), C.byref(off), xs.ctypes.data_as(u64p), xd.ctypes.data_as(u64p), C.byref(nx),
                                        C.byref(xt))
    if rc:
        raise ScalceError(f"[{rc}] scalce_shard_plan_own_pieces")
    return os_[: no.value].copy(), od[: no.value].copy(), int(ot.value), int(off.value), xs[: nx.value].copy(), xd[: nx.value].copy(), int(xt.value)


def shard_result_free(res):
    lib().scalce_shard_result_free(C.byref(res))


def entropy_begin_group(batches, prep_stream=0, stream=0, last=False):
    """ONE coder launch over the blocks of several shards (scalce_batch_entropy_begin_group); each shard is completed
    by its own entropy_end / finish on `stream`.  last: 1 / True = nothing will be queued behind this launch (the end of a
    run); 0 / False = more launches follow."""
    arr = (C.c_void_p * len(batches))(*[b.h for b in batches])
    batches[0]._check(batches[0].L.scalce_batch_entropy_begin_group_last(arr, len(batches), prep_stream, stream, int(last)))


class StreamStats(C.Structure):
    _fields_ = [("total_s", C.c_double), ("read_wait_s", C.c_double), ("h2d_wait_s", C.c_double), ("front_s", C.c_double),
                ("order_s", C.c_double), ("emit_s", C.c_double), ("entropy_s", C.c_double), ("rounds", C.c_uint64),
                ("reads", C.c_uint64), ("bytes", C.c_uint64 * 2),
                # STREAM_DIGEST: zlib's CRC-32 of each mate stream's text as the run read it (bytes[] says how long it was)
                ("crc", C.c_uint32 * 2)]


READ_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64)
STREAM_LEAN, STREAM_DEFER_ENTROPY = 1, 2
STREAM_DIGEST = 64  # SCALCE_STREAM_DIGEST


def stream_compress(ctx, params, read1, read2=None, piece_bytes=0, reads_hint=0, flags=0):
    """scalce_stream_compress: read1 / read2 are callables (cap) -> bytes (b"" at the end of the stream; raise for a read
    error), called from the library's reader threads.  Returns (Batch holding the results, StreamStats)."""
    def wrap(fn):
        def cb(_user, dst, cap):
            try:
                data = fn(int(cap))
            except Exception:  # noqa: BLE001 - reported to the library as a read error
                return -1
            if data:
                C.memmove(dst, data, len(data))
            return len(data)
        return READ_FN(cb)
    cb1 = wrap(read1)
    cb2 = wrap(read2) if read2 is not None else C.cast(None, READ_FN)
    out, st = C.c_void_p(), StreamStats()
    msg = C.create_string_buffer(512)
    L = ctx.L
    L.scalce_stream_compress.argtypes = [C.c_void_p, C.POINTER(Params), READ_FN, C.c_void_p, READ_FN, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                         C.POINTER(C.c_void_p), C.POINTER(StreamStats), C.c_char_p, C.c_size_t]
    rc = L.scalce_stream_compress(ctx.h, C.byref(params), cb1, None, cb2, None, int(piece_bytes), int(reads_hint), int(flags), C.byref(out),
                                  C.byref(st), msg, len(msg))
    if rc:
        raise ScalceError(f"[{rc}] " + msg.value.decode(errors="replace"))
    b = Batch.__new__(Batch)
    b.ctx, b.L, b.params, b.h, b.workspace = ctx, L, params, out, None
    return b, st


SKIP_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_uint64)


class UnpackParams(C.Structure):
    _fields_ = [("mates", C.c_int32), ("interleave", C.c_int32), ("no_qualities", C.c_int32), ("mate_digit", C.c_int32),
                ("ignore_names", C.c_int32), ("split", C.c_int32), ("library", C.c_char_p), ("window_text_bytes", C.c_uint64),
                # the length stream of a variable-length archive, per mate (all null: reads of one length)
                ("len_rd", READ_FN * 2), ("len_user", C.c_void_p * 2), ("len_skip", SKIP_FN * 2)]


class UnpackParamsDigest(UnpackParams):
    """scalce_unpack_params whole, as the library reads it: UnpackParams and, appended, `digest` -- != 0: the CRC-32 of the text
    handed to wr is taken on the device (UnpackStats.crc / .text_bytes).  What _unpack_params makes; it passes for an UnpackParams."""
    _fields_ = [("digest", C.c_int32)]


class UnpackStats(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("window_text_bytes", C.c_uint64), ("peak_device_bytes", C.c_uint64),
                ("pinned_host_bytes", C.c_uint64), ("records", C.c_uint64 * 2), ("total_s", C.c_double), ("setup_s", C.c_double),
                ("read_wait_s", C.c_double), ("decode_s", C.c_double), ("records_s", C.c_double), ("write_wait_s", C.c_double),
                ("write_s", C.c_double), ("error_mate", C.c_int32), ("error_stream", C.c_int32), ("error_wants_file", C.c_int32),
                ("decode_batches", C.c_uint64 * 2), ("crc", C.c_uint32 * 2), ("text_bytes", C.c_uint64 * 2)]


WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64))
UNPACK_LOOKAHEAD_BYTES = 1 << 20  # SCALCE_UNPACK_LOOKAHEAD_BYTES: what a stream may be read ahead of what the session has used


class UnpackRange(C.Structure):
    _fields_ = [("first_record", C.c_uint64), ("nrecords", C.c_uint64), ("skip", (SKIP_FN * 3) * 2)]


class UnpackRangeStats(C.Structure):
    _fields_ = [("first_record", C.c_uint64), ("nrecords", C.c_uint64), ("total_records", C.c_uint64),
                ("frames_decoded", C.c_uint64 * 2), ("frames_passed", C.c_uint64 * 2), ("symbols_decoded", C.c_uint64 * 2),
                ("bytes_delivered", (C.c_uint64 * 3) * 2), ("bytes_skipped", (C.c_uint64 * 3) * 2)]


def varlen_sample(text, sample=100000, stride=1, first=0, max_length=0):
    """scalce_varlen_sample (no device): (records sampled, read length, quality histogram) of the first `sample` records r of
    `text` with r % stride == first -- the read length a variable-length run is padded to is the longest sequence line among
    them, or max_length when that is given."""
    L = lib()
    L.scalce_varlen_sample.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]
    L.scalce_varlen_sample.restype = C.c_int64
    stat = (C.c_int32 * 128)()
    rl = C.c_int32(0)
    text = bytes(text)
    n = L.scalce_varlen_sample(text, len(text), int(sample), int(stride), int(first), int(max_length), stat, C.byref(rl))
    return int(n), int(rl.value), np.array(stat[:], dtype=np.int64)


def fastq_strip_window(ctx, read_len, nrecords, d_text, d_record_offsets, d_entries, entry_width, d_out, d_out_offsets, d_scan_ws,
                       stream=0):
    """scalce_fastq_strip_window: the pad out of a window of a variable-length archive (device pointers; see the header)."""
    L = ctx.L
    L.scalce_fastq_strip_window.argtypes = [C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    L.scalce_fastq_strip_window.restype = C.c_int
    ctx._check(L.scalce_fastq_strip_window(ctx.h, int(read_len), int(nrecords), d_text, d_record_offsets, d_entries, int(entry_width),
                                           d_out, d_out_offsets, d_scan_ws, stream))


def fastq_strip_ws_bytes(nrecords):
    L = lib()
    L.scalce_fastq_strip_ws_bytes.argtypes = [C.c_uint64]
    L.scalce_fastq_strip_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_strip_ws_bytes(int(nrecords)))


def range_plan_quality(read_len, first, n, total_syms):
    """scalce_range_plan_quality: (first frame, frames, symbols dropped in front, symbols behind them) of records
    [first, first + n) -- n None: to the end -- over a coded quality stream of total_syms symbols."""
    L = lib()
    L.scalce_range_plan_quality.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.scalce_range_plan_quality.restype = C.c_int
    out = (C.c_uint64 * 4)()
    rc = L.scalce_range_plan_quality(int(read_len), int(first), (1 << 64) - 1 if n is None else int(n), int(total_syms), out)
    if rc:
        raise ScalceError(f"[{rc}] scalce_range_plan_quality")
    return tuple(int(v) for v in out)


# what stream_decompress and stream_decompress_restore share: their callbacks over Python callables (`keep` holds them
# alive for the call), their UnpackParams and their error
def _unpack_read_fn(keep, fn):
    def cb(_user, dst, cap):
        try:
            data = fn(int(cap))
        except Exception:  # noqa: BLE001 - reported to the library as a read error
            return -1
        if data:
            C.memmove(dst, data, len(data))
        return len(data)
    keep.append(READ_FN(cb))
    return keep[-1]


def _unpack_skip_fn(keep, fn):
    def cb(_user, nbytes):
        try:
            return int(fn(int(nbytes)))
        except Exception:  # noqa: BLE001 - reported to the library as a read error
            return -1
    keep.append(SKIP_FN(cb))
    return keep[-1]


def _unpack_write_fn(write):
    def wcb(_user, mate, first, nrec, text, nbytes, roff):
        try:
            offs = [roff[i] for i in range(nrec + 1)] if roff else None
            write(int(mate), int(first), int(nrec), C.string_at(text, nbytes), offs)
        except Exception:  # noqa: BLE001 - reported to the library as a failed write
            return 1
        return 0
    return WRITE_FN(wcb)


def _unpack_params(mates, interleave, no_qualities, mate_digit, library, split, window_text_bytes):
    return UnpackParamsDigest(mates, int(interleave), int(no_qualities), int(mates == 2 if mate_digit is None else mate_digit),
                        int(library is not None), int(split), library.encode() if library is not None else None, int(window_text_bytes))


def _unpack_check(rc, msg):
    if rc:
        raise ScalceError(f"[{rc}] " + msg.value.decode(errors="replace"))


class UnpackComments(C.Structure):
    """scalce_unpack_comments: the comment streams of an archive made with --keep-comments, one per mate"""
    _fields_ = [("com_rd", READ_FN * 2), ("com_user", C.c_void_p * 2)]


def _unpack_comments(keep, mates, comment_readers):
    cm = UnpackComments()
    for m in range(mates):
        if comment_readers[m] is not None:
            cm.com_rd[m] = _unpack_read_fn(keep, comment_readers[m])
    return cm


class UnpackExceptions(C.Structure):
    """scalce_unpack_exceptions: the exception streams of an archive made with --keep-bases, one per mate"""
    _fields_ = [("exc_rd", READ_FN * 2), ("exc_user", C.c_void_p * 2)]


def _unpack_exceptions(keep, mates, exception_readers):
    ex = UnpackExceptions()
    for m in range(mates):
        if exception_readers[m] is not None:
            ex.exc_rd[m] = _unpack_read_fn(keep, exception_readers[m])
    return ex


class UnpackPlus(C.Structure):
    """scalce_unpack_plus: the plus-line streams of an archive made with --keep-plus, one per mate"""
    _fields_ = [("plus_rd", READ_FN * 2), ("plus_user", C.c_void_p * 2)]


def _unpack_plus(keep, mates, plus_readers):
    pl = UnpackPlus()
    for m in range(mates):
        if plus_readers[m] is not None:
            pl.plus_rd[m] = _unpack_read_fn(keep, plus_readers[m])
    return pl


def _decompress_streams(ctx, p, cm, rg, rp, rd, user, wfn, st, rst, ost, msg, ex=None, pl=None):
    """The one entry point behind the three shapes of decompression for archives with side streams: cm the comment streams
    (scalce_stream_decompress_comments), ex the exception streams beside them or alone (scalce_stream_decompress_exceptions),
    pl the plus-line streams beside either or alone (scalce_stream_decompress_plus)"""
    L = ctx.L
    if pl is not None:
        L.scalce_stream_decompress_plus.argtypes = [C.c_void_p, C.POINTER(UnpackParams), C.POINTER(UnpackComments), C.POINTER(UnpackExceptions),
                                                    C.POINTER(UnpackPlus), C.POINTER(UnpackRange), C.POINTER(RestoreParams), C.c_void_p,
                                                    C.c_void_p, WRITE_FN, C.c_void_p, C.POINTER(UnpackStats), C.POINTER(UnpackRangeStats),
                                                    C.POINTER(RestoreStats), C.c_char_p, C.c_size_t]
        L.scalce_stream_decompress_plus.restype = C.c_int
        return L.scalce_stream_decompress_plus(ctx.h, C.byref(p), C.byref(cm) if cm is not None else None,
                                               C.byref(ex) if ex is not None else None, C.byref(pl),
                                               C.byref(rg) if rg is not None else None, C.byref(rp) if rp is not None else None,
                                               C.cast(rd, C.c_void_p), C.cast(user, C.c_void_p), wfn, None, C.byref(st),
                                               C.byref(rst) if rst is not None else None, C.byref(ost) if ost is not None else None,
                                               msg, len(msg))
    if ex is not None:
        L.scalce_stream_decompress_exceptions.argtypes = [C.c_void_p, C.POINTER(UnpackParams), C.POINTER(UnpackComments), C.POINTER(UnpackExceptions),
                                                          C.POINTER(UnpackRange), C.POINTER(RestoreParams), C.c_void_p, C.c_void_p, WRITE_FN,
                                                          C.c_void_p, C.POINTER(UnpackStats), C.POINTER(UnpackRangeStats), C.POINTER(RestoreStats),
                                                          C.c_char_p, C.c_size_t]
        L.scalce_stream_decompress_exceptions.restype = C.c_int
        return L.scalce_stream_decompress_exceptions(ctx.h, C.byref(p), C.byref(cm) if cm is not None else None, C.byref(ex),
                                                     C.byref(rg) if rg is not None else None, C.byref(rp) if rp is not None else None,
                                                     C.cast(rd, C.c_void_p), C.cast(user, C.c_void_p), wfn, None, C.byref(st),
                                                     C.byref(rst) if rst is not None else None, C.byref(ost) if ost is not None else None,
                                                     msg, len(msg))
    L.scalce_stream_decompress_comments.argtypes = [C.c_void_p, C.POINTER(UnpackParams), C.POINTER(UnpackComments), C.POINTER(UnpackRange),
                                                    C.POINTER(RestoreParams), C.c_void_p, C.c_void_p, WRITE_FN, C.c_void_p,
                                                    C.POINTER(UnpackStats), C.POINTER(UnpackRangeStats), C.POINTER(RestoreStats),
                                                    C.c_char_p, C.c_size_t]
    L.scalce_stream_decompress_comments.restype = C.c_int
    return L.scalce_stream_decompress_comments(ctx.h, C.byref(p), C.byref(cm) if cm is not None else None,
                                               C.byref(rg) if rg is not None else None, C.byref(rp) if rp is not None else None,
                                               C.cast(rd, C.c_void_p), C.cast(user, C.c_void_p), wfn, None, C.byref(st),
                                               C.byref(rst) if rst is not None else None, C.byref(ost) if ost is not None else None,
                                               msg, len(msg))


def stream_decompress(ctx, readers, write, mates=1, interleave=False, no_qualities=False, mate_digit=None, library=None,
                      split=0, window_text_bytes=0, first_record=0, nrecords=None, skippers=None, length_readers=None,
                      length_skippers=None, comment_readers=None, exception_readers=None, plus_readers=None, digest=False):
    """digest: the CRC-32 of the text handed to `write` is taken on the device: the stats' crc / text_bytes, per mate.
    scalce_stream_decompress_range: an archive, or a range of its records, back to text in windows of whole records.
    readers[m] = the three callables (cap) -> bytes of mate m's .scalcer, .scalcen and .scalceq streams (b"" at the end; raise
    for a read error); write(mate, first_record, nrecords, text_bytes, record_offsets or None) receives every window in
    order, from the library's writer thread (raise to end the session).  library: print names as <library>.<index> whatever
    the archive holds (-n).  first_record / nrecords (None: to the end): the range, in archive order; skippers[m] = three
    callables (nbytes) -> bytes passed over, or None where the stream can only be read.  length_readers[m] (and, optionally,
    length_skippers[m]): the .scalcel stream of a variable-length archive, one callable per mate.  Returns UnpackStats; its attribute
    `range` holds the UnpackRangeStats of the run.  comment_readers[m]: the .scalcec stream of an archive made with
    --keep-comments, one callable per mate -- the call then goes through scalce_stream_decompress_comments.  exception_readers[m]:
    the .scalcex stream of an archive made with --keep-bases -- through scalce_stream_decompress_exceptions.  plus_readers[m]:
    the .scalcep stream of an archive made with --keep-plus -- through scalce_stream_decompress_plus."""
    keep = []
    wfn = _unpack_write_fn(write)
    rd = ((READ_FN * 3) * 2)()
    user = ((C.c_void_p * 3) * 2)()
    rg = UnpackRange(int(first_record), (1 << 64) - 1 if nrecords is None else int(nrecords))
    for m in range(mates):
        for k in range(3):
            if readers[m][k] is not None:
                rd[m][k] = _unpack_read_fn(keep, readers[m][k])
            if skippers is not None and skippers[m] is not None and skippers[m][k] is not None:
                rg.skip[m][k] = _unpack_skip_fn(keep, skippers[m][k])
    p = _unpack_params(mates, interleave, no_qualities, mate_digit, library, split, window_text_bytes)
    p.digest = int(bool(digest))
    for m in range(mates):
        if length_readers is not None and length_readers[m] is not None:
            p.len_rd[m] = _unpack_read_fn(keep, length_readers[m])
        if length_skippers is not None and length_skippers[m] is not None:
            p.len_skip[m] = _unpack_skip_fn(keep, length_skippers[m])
    st = UnpackStats()
    rst = UnpackRangeStats()
    msg = C.create_string_buffer(1024)
    L = ctx.L
    L.scalce_stream_decompress_range.argtypes = [C.c_void_p, C.POINTER(UnpackParams), C.POINTER(UnpackRange), C.c_void_p, C.c_void_p,
                                                 WRITE_FN, C.c_void_p, C.POINTER(UnpackStats), C.POINTER(UnpackRangeStats), C.c_char_p,
                                                 C.c_size_t]
    L.scalce_stream_decompress_range.restype = C.c_int
    if plus_readers is not None:
        cm = _unpack_comments(keep, mates, comment_readers) if comment_readers is not None else None
        ex = _unpack_exceptions(keep, mates, exception_readers) if exception_readers is not None else None
        rc = _decompress_streams(ctx, p, cm, rg, None, rd, user, wfn, st, rst, None, msg, ex=ex, pl=_unpack_plus(keep, mates, plus_readers))
    elif exception_readers is not None:
        cm = _unpack_comments(keep, mates, comment_readers) if comment_readers is not None else None
        rc = _decompress_streams(ctx, p, cm, rg, None, rd, user, wfn, st, rst, None, msg, ex=_unpack_exceptions(keep, mates, exception_readers))
    elif comment_readers is not None:
        rc = _decompress_streams(ctx, p, _unpack_comments(keep, mates, comment_readers), rg, None, rd, user, wfn, st, rst, None, msg)
    else:
        rc = L.scalce_stream_decompress_range(ctx.h, C.byref(p), C.byref(rg), C.cast(rd, C.c_void_p), C.cast(user, C.c_void_p), wfn, None,
                                              C.byref(st), C.byref(rst), msg, len(msg))
    _unpack_check(rc, msg)
    st.range = rst
    return st


# ---- the input order back (archives made with --keep-order) -----------------------------------------------------------------
ORDER_HEADER_BYTES = 24  # the 8 magic bytes, int32 4 (entry width), int32 0, int64 N; then N x u32
ORDER_MAX_STRIPES = 65536
STREAM_KEEP_ORDER = 4    # SCALCE_STREAM_KEEP_ORDER


def pack_order(perm):
    """The bytes of a .scalceo stream: header, then the input index of the k-th record of the archive."""
    perm = np.asarray(perm, dtype=np.int64)
    if perm.size and (perm.min() < 0 or perm.max() > 0xFFFFFFFF):
        raise ValueError("an entry of an order stream is an unsigned 32-bit index")
    return b"scalce22" + struct.pack("<iiq", 4, 0, perm.size) + perm.astype("<u4").tobytes()


def unpack_order(data):
    """The entries of the bytes of a .scalceo stream (out of its container); ValueError with the library's message."""
    if len(data) < ORDER_HEADER_BYTES:
        raise ValueError("truncated order stream")
    width, zero, n = struct.unpack("<iiq", data[8:24])
    if data[:7] != b"scalce2" or width != 4 or zero != 0 or n < 0 or n > 0xFFFFFFFF:
        raise ValueError("is not a scalce order stream")
    if len(data) < ORDER_HEADER_BYTES + 4 * n:
        raise ValueError("truncated order stream")
    if len(data) != ORDER_HEADER_BYTES + 4 * n:
        raise ValueError(f"order stream holds {(len(data) - ORDER_HEADER_BYTES) // 4} entries, its header says {n}")
    return np.frombuffer(data, dtype="<u4", offset=ORDER_HEADER_BYTES).astype(np.int64)


def order_plan(total_records, window_text_bytes, max_record_bytes):
    """scalce_order_plan (no device): (R, S) -- records per stripe and stripes of the order restore."""
    L = lib()
    L.scalce_order_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.scalce_order_plan.restype = C.c_int
    out = (C.c_uint64 * 2)()
    rc = L.scalce_order_plan(int(total_records), int(window_text_bytes), int(max_record_bytes), out)
    if rc:
        raise ScalceError(f"[{rc}] scalce_order_plan")
    return int(out[0]), int(out[1])


def records_permute_ws_bytes(nrecords):
    L = lib()
    L.scalce_records_permute_ws_bytes.argtypes = [C.c_uint64]
    L.scalce_records_permute_ws_bytes.restype = C.c_uint64
    return int(L.scalce_records_permute_ws_bytes(int(nrecords)))


def records_permute(ctx, d_text, d_record_offsets, nrecords, text_bytes, d_source, d_out, out_cap, d_out_offsets, d_ws, stream=0):
    """scalce_records_permute: output record r is input record d_source[r] (device pointers; see the header)."""
    L = ctx.L
    L.scalce_records_permute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.scalce_records_permute.restype = C.c_int
    ctx._check(L.scalce_records_permute(ctx.h, d_text, d_record_offsets, int(nrecords), int(text_bytes), d_source, d_out, int(out_cap),
                                        d_out_offsets, d_ws, stream))


def order_group_ws_bytes(nrecords, nstripes):
    L = lib()
    L.scalce_order_group_ws_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.scalce_order_group_ws_bytes.restype = C.c_uint64
    return int(L.scalce_order_group_ws_bytes(int(nrecords), int(nstripes)))


def order_group(ctx, d_index, nrecords, stripe_records, total_records, nstripes, d_source, d_stripe_counts, d_bad, d_ws, stream=0):
    """scalce_order_group: a window's records grouped by the stripe of their entry, stable (device pointers)."""
    L = ctx.L
    L.scalce_order_group.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint64] * 4 + [C.c_void_p] * 5
    L.scalce_order_group.restype = C.c_int
    ctx._check(L.scalce_order_group(ctx.h, d_index, int(nrecords), int(stripe_records), int(total_records), int(nstripes), d_source,
                                    d_stripe_counts, d_bad, d_ws, stream))


def order_place(ctx, d_index, m, base, expect, d_source, d_bad, stream=0):
    """scalce_order_place: d_source[d_index[i] - base] = i, checked by scatter and verify (device pointers)."""
    L = ctx.L
    L.scalce_order_place.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint64] * 3 + [C.c_void_p] * 3
    L.scalce_order_place.restype = C.c_int
    ctx._check(L.scalce_order_place(ctx.h, d_index, int(m), int(base), int(expect), d_source, d_bad, stream))


def order_gather(ctx, d_in, d_source, n, d_out, stream=0):
    L = ctx.L
    L.scalce_order_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.scalce_order_gather.restype = C.c_int
    ctx._check(L.scalce_order_gather(ctx.h, d_in, d_source, int(n), d_out, stream))


# ---- zlib's CRC-32 of device memory (--digest; kernels_crc.hpp) ---------------------------------------------------------------
def crc32_plan(nbytes):
    """scalce_crc32_plan (no device): (G, T, S, workgroups) -- bytes per lane per step, per workgroup step (tile), per workgroup
    (span) and the workgroups launched for a range of nbytes that begins on a 16-byte boundary."""
    L = lib()
    L.scalce_crc32_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint32)]
    L.scalce_crc32_plan.restype = C.c_int
    out = (C.c_uint32 * 4)()
    rc = L.scalce_crc32_plan(int(nbytes), out)
    if rc:
        raise ScalceError(f"[{rc}] scalce_crc32_plan")
    return tuple(int(v) for v in out)


def crc32_ws_bytes(nbytes):
    L = lib()
    L.scalce_crc32_ws_bytes.argtypes = [C.c_uint64]
    L.scalce_crc32_ws_bytes.restype = C.c_uint64
    return int(L.scalce_crc32_ws_bytes(int(nbytes)))


def crc32_combine(crc_a, crc_b, len_b):
    """scalce_crc32_combine (no device): crc32(A || B) from crc32(A), crc32(B) and len(B)."""
    L = lib()
    L.scalce_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.scalce_crc32_combine.restype = C.c_uint32
    return int(L.scalce_crc32_combine(int(crc_a), int(crc_b), int(len_b)))


def crc32_device(ctx, d_data, nbytes, d_crc, d_ws, stream=0):
    """scalce_crc32_device: enqueues zlib's crc32 of nbytes at d_data (any byte address) into the u32 at d_crc (device pointers)."""
    L = ctx.L
    L.scalce_crc32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scalce_crc32_device.restype = C.c_int
    ctx._check(L.scalce_crc32_device(ctx.h, d_data, int(nbytes), d_crc, d_ws, stream))


# ---- what follows the names (archives made with --keep-comments) ------------------------------------------------------------
COMMENT_HEADER_BYTES = 24  # the 8 magic bytes, int32 0 (text entries), int32 C (longest entry), int64 N; then N entries + newline
COMMENT_MAX_ENTRY = 65535
STREAM_KEEP_COMMENTS = 8   # SCALCE_STREAM_KEEP_COMMENTS


def pack_comments(entries):
    """The bytes of a .scalcec stream: header, then every entry (bytes, no newline inside) followed by a newline."""
    entries = [bytes(e) for e in entries]
    for e in entries:
        if b"\n" in e:
            raise ValueError("an entry of a comment stream holds no newline")
        if len(e) > COMMENT_MAX_ENTRY:
            raise ValueError("an entry of a comment stream is at most 65535 bytes long")
    longest = max((len(e) for e in entries), default=0)
    return b"scalce22" + struct.pack("<iiq", 0, longest, len(entries)) + b"".join(e + b"\n" for e in entries)


def unpack_comments(data):
    """The entries of the bytes of a .scalcec stream (out of its container); ValueError with the library's message."""
    data = bytes(data)
    if len(data) < COMMENT_HEADER_BYTES:
        raise ValueError("truncated comment stream")
    width, longest, n = struct.unpack("<iiq", data[8:24])
    if data[:7] != b"scalce2" or width != 0 or longest < 0 or longest > COMMENT_MAX_ENTRY or n < 0 or n > 0xFFFFFFFF:
        raise ValueError("is not a scalce comment stream")
    body = data[COMMENT_HEADER_BYTES:]
    entries = body.split(b"\n")
    if entries.pop() != b"" or len(entries) < n:  # (the stream ends inside an entry, or before N entries)
        raise ValueError("truncated comment stream")
    if len(entries) != n:
        raise ValueError(f"comment stream holds {len(entries)} entries, its header says {n}")
    if any(len(e) > longest for e in entries):
        raise ValueError("comment stream: an entry is longer than its header says")
    return entries


def fastq_comment_ws_bytes(nrecords, entry_bytes):
    L = lib()
    L.scalce_fastq_comment_ws_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.scalce_fastq_comment_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_comment_ws_bytes(int(nrecords), int(entry_bytes)))


def fastq_comment_window(ctx, read_len, has_qualities, nrecords, d_text, d_record_offsets, d_entries, entry_bytes, d_out,
                         d_out_offsets, d_bad, d_ws, stream=0):
    """scalce_fastq_comment_window: a window's entries back between each name and its newline (device pointers; see the header)."""
    L = ctx.L
    L.scalce_fastq_comment_window.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 5
    L.scalce_fastq_comment_window.restype = C.c_int
    ctx._check(L.scalce_fastq_comment_window(ctx.h, int(read_len), int(bool(has_qualities)), int(nrecords), d_text, d_record_offsets,
                                             d_entries, int(entry_bytes), d_out, d_out_offsets, d_bad, d_ws, stream))


def fastq_comment_pairs_ws_bytes(npairs, entry_bytes):
    L = lib()
    L.scalce_fastq_comment_pairs_ws_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.scalce_fastq_comment_pairs_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_comment_pairs_ws_bytes(int(npairs), int(entry_bytes)))


def fastq_comment_window_pairs(ctx, read_lens, has_qualities, npairs, d_text, d_pair_offsets, d_name_off2, d_entries, entry_bytes, d_out,
                               d_out_pair_offsets, d_bad, d_ws, stream=0):
    """scalce_fastq_comment_window_pairs: the same for an interleaved window, both mates' entries pair by pair (device pointers)."""
    L = ctx.L
    L.scalce_fastq_comment_window_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 5
    L.scalce_fastq_comment_window_pairs.restype = C.c_int
    rl = (C.c_int * 2)(int(read_lens[0]), int(read_lens[1]))
    ctx._check(L.scalce_fastq_comment_window_pairs(ctx.h, rl, int(bool(has_qualities)), int(npairs), d_text, d_pair_offsets, d_name_off2,
                                                   d_entries, int(entry_bytes), d_out, d_out_pair_offsets, d_bad, d_ws, stream))


# ---- the letters and qualities the archive does not keep (archives made with --keep-bases) ------------------------------------
EXCEPTION_HEADER_BYTES = 32  # the 8 magic bytes, int32 8 (entry width), int32 L, int64 N (records), int64 X (entries); then X x u64
EXCEPTION_MAX_RECORDS = 1 << 36
STREAM_KEEP_BASES = 16       # SCALCE_STREAM_KEEP_BASES


def exception_entry(record, position, letter, quality=0):
    """One u64 of a .scalcex stream: bits 0-7 the letter, 8-15 the quality character, 16-27 the position, 28-63 the record."""
    return int(letter) | int(quality) << 8 | int(position) << 16 | int(record) << 28


def pack_exceptions(entries, read_len, nrecords):
    """The bytes of a .scalcex stream: header, then the entries (u64, strictly ascending) little-endian."""
    e = np.ascontiguousarray(entries, dtype="<u8").reshape(-1)
    if len(e) > 1 and not ((e[1:] >> np.uint64(16)) > (e[:-1] >> np.uint64(16))).all():   # (by record and position: one entry per place)
        raise ValueError("exception stream: entries are not in ascending order")
    return b"scalce22" + struct.pack("<iiqq", 8, int(read_len), int(nrecords), len(e)) + e.tobytes()


def unpack_exceptions(data):
    """(read_len, nrecords, entries as a u64 array) of the bytes of a .scalcex stream (out of its container); ValueError with
    the library's message."""
    data = bytes(data)
    if len(data) < EXCEPTION_HEADER_BYTES:
        raise ValueError("truncated exception stream")
    width, L, n, x = struct.unpack("<iiqq", data[8:32])
    if data[:7] != b"scalce2" or width != 8 or L <= 0 or L >= 4096 or n < 0 or n >= EXCEPTION_MAX_RECORDS or x < 0:
        raise ValueError("is not a scalce exception stream")
    if len(data) - EXCEPTION_HEADER_BYTES < 8 * x:
        raise ValueError("truncated exception stream")
    e = np.frombuffer(data, dtype="<u8", count=x, offset=EXCEPTION_HEADER_BYTES).astype(np.uint64)
    if len(e) > 1 and not ((e[1:] >> np.uint64(16)) > (e[:-1] >> np.uint64(16))).all():
        raise ValueError("exception stream: entries are not in ascending order")
    if len(e) and (((e >> np.uint64(28)) >= np.uint64(n)).any() or (((e >> np.uint64(16)) & np.uint64(0xFFF)) >= np.uint64(L)).any()):
        raise ValueError("exception stream: an entry lies outside its record")
    return L, n, e


def fastq_exception_window(ctx, read_len, has_qualities, first_record, nrecords, d_text, d_record_offsets, d_entries, nentries, d_bad,
                           stream=0):
    """scalce_fastq_exception_window: a window's entries of the exception stream back into its text, in place (device pointers)."""
    L = ctx.L
    L.scalce_fastq_exception_window.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 2
    L.scalce_fastq_exception_window.restype = C.c_int
    ctx._check(L.scalce_fastq_exception_window(ctx.h, int(read_len), int(bool(has_qualities)), int(first_record), int(nrecords), d_text,
                                               d_record_offsets, d_entries, int(nentries), d_bad, stream))


def fastq_exception_pairs_ws_bytes(npairs):
    L = lib()
    L.scalce_fastq_exception_pairs_ws_bytes.argtypes = [C.c_uint64]
    L.scalce_fastq_exception_pairs_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_exception_pairs_ws_bytes(int(npairs)))


def fastq_exception_window_pairs(ctx, read_lens, has_qualities, first_pair, npairs, d_text, d_pair_offsets, d_name_off2, d_entries, nentries,
                                 d_bad, d_ws, stream=0, library_len=0):
    """scalce_fastq_exception_window_pairs: the same for an interleaved window; d_entries / nentries: one per mate;
    d_name_off2 None: made-up names of a library name of library_len characters."""
    L = ctx.L
    L.scalce_fastq_exception_window_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3 + [
        C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)] + [C.c_void_p] * 3
    L.scalce_fastq_exception_window_pairs.restype = C.c_int
    rl = (C.c_int * 2)(int(read_lens[0]), int(read_lens[1]))
    de = (C.c_void_p * 2)(d_entries[0], d_entries[1])
    ne = (C.c_uint64 * 2)(int(nentries[0]), int(nentries[1]))
    ctx._check(L.scalce_fastq_exception_window_pairs(ctx.h, rl, int(bool(has_qualities)), int(first_pair), int(npairs), d_text, d_pair_offsets,
                                                     d_name_off2, int(library_len), de, ne, d_bad, d_ws, stream))


# ---- the '+' lines (archives made with --keep-plus; format.pack_plus / unpack_plus hold the stream's layout) ------------------
STREAM_KEEP_PLUS = 32  # SCALCE_STREAM_KEEP_PLUS


def fastq_plus_ws_bytes(nrecords, entry_bytes):
    L = lib()
    L.scalce_fastq_plus_ws_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.scalce_fastq_plus_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_plus_ws_bytes(int(nrecords), int(entry_bytes)))


def fastq_plus_window(ctx, nrecords, d_text, d_record_offsets, d_entries, entry_bytes, d_out, out_cap, d_out_offsets, d_bad, d_ws, stream=0):
    """scalce_fastq_plus_window: a window's '+' lines back behind each '+' (device pointers; see the header)."""
    L = ctx.L
    L.scalce_fastq_plus_window.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
    L.scalce_fastq_plus_window.restype = C.c_int
    ctx._check(L.scalce_fastq_plus_window(ctx.h, int(nrecords), d_text, d_record_offsets, d_entries, int(entry_bytes), d_out, int(out_cap),
                                          d_out_offsets, d_bad, d_ws, stream))


def fastq_plus_pairs_ws_bytes(npairs, entry_bytes):
    L = lib()
    L.scalce_fastq_plus_pairs_ws_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.scalce_fastq_plus_pairs_ws_bytes.restype = C.c_uint64
    return int(L.scalce_fastq_plus_pairs_ws_bytes(int(npairs), int(entry_bytes)))


def fastq_plus_window_pairs(ctx, read_lens, npairs, d_text, d_pair_offsets, d_entries, entry_bytes, d_out, out_cap, d_out_pair_offsets, d_bad,
                            d_ws, stream=0):
    """scalce_fastq_plus_window_pairs: the same for an interleaved window, both mates' entries pair by pair (device pointers)."""
    L = ctx.L
    L.scalce_fastq_plus_window_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_uint64] + [C.c_void_p] * 3 + [
        C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
    L.scalce_fastq_plus_window_pairs.restype = C.c_int
    rl = (C.c_int * 2)(int(read_lens[0]), int(read_lens[1]))
    ctx._check(L.scalce_fastq_plus_window_pairs(ctx.h, rl, int(npairs), d_text, d_pair_offsets, d_entries, int(entry_bytes), d_out,
                                                int(out_cap), d_out_pair_offsets, d_bad, d_ws, stream))


class RestoreParams(C.Structure):
    _fields_ = [("order_rd", READ_FN * 2), ("order_user", C.c_void_p * 2), ("spill_dir", C.c_char_p)]


class RestoreStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("stripes", C.c_uint64), ("stripe_records", C.c_uint64), ("spilled_bytes", C.c_uint64),
                ("group_pass_s", C.c_double), ("stripe_pass_s", C.c_double), ("spill_write_s", C.c_double),
                ("spill_read_s", C.c_double), ("place_wait_s", C.c_double)]


def stream_decompress_restore(ctx, readers, order_readers, write, spill_dir, mates=1, interleave=False, no_qualities=False,
                              mate_digit=None, library=None, split=0, window_text_bytes=0, length_readers=None, comment_readers=None,
                              exception_readers=None, plus_readers=None, digest=False):
    """digest: as for stream_decompress.
    scalce_stream_decompress_restore: stream_decompress with the input order restored.  order_readers[m]: the callable
    (cap) -> bytes of the .scalceo stream, read from its start once per mate pass (interleaved: only [0]); write receives
    the text in input order, one stripe per call, first_record = the input index of its first record.  Returns
    UnpackStats; its attribute `restore` holds the RestoreStats."""
    keep = []
    wfn = _unpack_write_fn(write)
    rd = ((READ_FN * 3) * 2)()
    user = ((C.c_void_p * 3) * 2)()
    for m in range(mates):
        for k in range(3):
            if readers[m][k] is not None:
                rd[m][k] = _unpack_read_fn(keep, readers[m][k])
    p = _unpack_params(mates, interleave, no_qualities, mate_digit, library, split, window_text_bytes)
    p.digest = int(bool(digest))
    rp = RestoreParams()
    rp.spill_dir = os.fsencode(spill_dir)
    for m in range(1 if interleave else mates):
        rp.order_rd[m] = _unpack_read_fn(keep, order_readers[m])
        if length_readers is not None and length_readers[m] is not None:
            p.len_rd[m] = _unpack_read_fn(keep, length_readers[m])
    st = UnpackStats()
    rst = RestoreStats()
    msg = C.create_string_buffer(1024)
    L = ctx.L
    L.scalce_stream_decompress_restore.argtypes = [C.c_void_p, C.POINTER(UnpackParams), C.POINTER(RestoreParams), C.c_void_p, C.c_void_p,
                                                   WRITE_FN, C.c_void_p, C.POINTER(UnpackStats), C.POINTER(RestoreStats), C.c_char_p,
                                                   C.c_size_t]
    L.scalce_stream_decompress_restore.restype = C.c_int
    if plus_readers is not None:
        cm = _unpack_comments(keep, mates, comment_readers) if comment_readers is not None else None
        ex = _unpack_exceptions(keep, mates, exception_readers) if exception_readers is not None else None
        rc = _decompress_streams(ctx, p, cm, None, rp, rd, user, wfn, st, None, rst, msg, ex=ex, pl=_unpack_plus(keep, mates, plus_readers))
    elif exception_readers is not None:
        cm = _unpack_comments(keep, mates, comment_readers) if comment_readers is not None else None
        rc = _decompress_streams(ctx, p, cm, None, rp, rd, user, wfn, st, None, rst, msg, ex=_unpack_exceptions(keep, mates, exception_readers))
    elif comment_readers is not None:
        rc = _decompress_streams(ctx, p, _unpack_comments(keep, mates, comment_readers), None, rp, rd, user, wfn, st, None, rst, msg)
    else:
        rc = L.scalce_stream_decompress_restore(ctx.h, C.byref(p), C.byref(rp), C.cast(rd, C.c_void_p), C.cast(user, C.c_void_p), wfn, None,
                                                C.byref(st), C.byref(rst), msg, len(msg))
    _unpack_check(rc, msg)
    st.restore = rst
    return st


class Workspace:
    """Front-stage device buffers shared by several batches (scalce_workspace): see include/scalce_hip.h."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._check(ctx.L.scalce_workspace_create(ctx.h, C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.L.scalce_workspace_destroy(self.h)
            self.h = C.c_void_p()


class Batch:
    """One FASTQ shard in HBM (scalce_batch)."""

    def __init__(self, ctx, read_len, max_reads, max_text, paired=False, use_names=True, no_ac=False, qmap=None,
                 bucket_set_size=0, read_len2=0, qprev=None, workspace=None, fasta=False, no_qualities=False, interleaved=False,
                 variable_length=False, keep_comments=False, keep_bases=False, keep_plus=False):
        self.ctx = ctx
        self.L = ctx.L
        p = Params()
        self.L.scalce_params_default(C.byref(p))
        p.read_len[0] = int(read_len)
        p.read_len[1] = int(read_len2 or read_len) if paired else 0
        p.paired, p.use_names, p.no_ac = int(paired), int(use_names), int(no_ac)
        p.bucket_set_size = int(bucket_set_size)
        p.fasta, p.no_qualities = int(fasta), int(no_qualities)  # two-line records (-f) / qualities dropped (-Q)
        p.interleaved = int(interleaved)  # -i: one text, mate 1 and mate 2 of a pair one after the other (needs paired)
        p.variable_length = int(variable_length)  # reads of 0 .. read_len bases, padded to read_len in front of the ingest
        if qmap is not None:  # [(offset, values)] per mate
            for m, (off, vals) in enumerate(qmap):
                p.qmap[m].offset = int(off)
                for i in range(128):
                    p.qmap[m].values[i] = int(vals[i])
        if qprev is not None:
            for m in range(2):
                for i in range(2):
                    p.qprev[m][i] = int(qprev[m][i])
        self.params = p
        self.h = C.c_void_p()
        self.workspace = workspace  # keeps it alive
        if workspace is not None:
            rc = self.L.scalce_batch_create_shared(ctx.h, C.byref(p), int(max_reads), int(max_text), workspace.h, C.byref(self.h))
        else:
            rc = self.L.scalce_batch_create(ctx.h, C.byref(p), int(max_reads), int(max_text), C.byref(self.h))
        if rc:
            raise ScalceError(f"[{rc}] " + self.L.scalce_last_error(ctx.h).decode())
        if keep_comments:
            self.set_keep_comments(True)
        if keep_bases:
            self.set_keep_bases(True)
        if keep_plus:
            self.set_keep_plus(True)

    def _check(self, rc):
        self.ctx._check(rc)

    def ingest(self, mate, d_text, nbytes, stream=0):
        self._check(self.L.scalce_batch_ingest(self.h, mate, d_text, int(nbytes), stream))

    def append(self, d_text1, n1, d_text2=None, n2=0, final=False, stream=0, flags=0):
        """Next piece of the read stream behind the rows already held; returns the bytes consumed per mate.
        flags: APPEND_NO_QUALITY / APPEND_NO_TOKENIZE beside `final` (APPEND_FINAL)."""
        used = (C.c_uint64 * 2)()
        self._check(self.L.scalce_batch_append(self.h, d_text1, int(n1), d_text2, int(n2), int(bool(final)) | int(flags), used, stream))
        return used[0], used[1]

    def reset(self):
        self._check(self.L.scalce_batch_reset(self.h))

    def set_lean(self, lean=True):
        self.L.scalce_batch_set_lean(self.h, int(lean))

    def set_keep_order(self, on=True):
        """OUT_PERM stays valid behind emit() and finish(), lean or not (scalce_batch_set_keep_order)."""
        self.L.scalce_batch_set_keep_order.argtypes = [C.c_void_p, C.c_int]
        self._check(self.L.scalce_batch_set_keep_order(self.h, int(on)))

    def set_keep_comments(self, on=True):
        """What follows the names becomes OUT_COMMENTS (scalce_batch_set_keep_comments): before the run's first ingest or append."""
        self.L.scalce_batch_set_keep_comments.argtypes = [C.c_void_p, C.c_int]
        self.L.scalce_batch_set_keep_comments.restype = C.c_int
        self._check(self.L.scalce_batch_set_keep_comments(self.h, int(on)))

    def comments_info(self, mate=0):
        """scalce_batch_comments_info: (bytes of OUT_COMMENTS, longest entry) of `mate`."""
        self.L.scalce_batch_comments_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        self.L.scalce_batch_comments_info.restype = C.c_int
        n, c = C.c_uint64(0), C.c_uint32(0)
        self._check(self.L.scalce_batch_comments_info(self.h, int(mate), C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def set_keep_plus(self, on=True):
        """Every record's '+' line becomes OUT_PLUS (scalce_batch_set_keep_plus): before the run's first ingest or append."""
        self.L.scalce_batch_set_keep_plus.argtypes = [C.c_void_p, C.c_int]
        self.L.scalce_batch_set_keep_plus.restype = C.c_int
        self._check(self.L.scalce_batch_set_keep_plus(self.h, int(on)))

    def plus_info(self, mate=0):
        """scalce_batch_plus_info: (bytes of OUT_PLUS, longest stored entry, repeats, literals) of `mate`."""
        self.L.scalce_batch_plus_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]
        self.L.scalce_batch_plus_info.restype = C.c_int
        n, p, r, l = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.scalce_batch_plus_info(self.h, int(mate), C.byref(n), C.byref(p), C.byref(r), C.byref(l)))
        return int(n.value), int(p.value), int(r.value), int(l.value)

    def set_keep_bases(self, on=True):
        """The letters and qualities the archive does not keep become OUT_EXCEPTIONS (scalce_batch_set_keep_bases): before the
        run's first ingest or append."""
        self.L.scalce_batch_set_keep_bases.argtypes = [C.c_void_p, C.c_int]
        self.L.scalce_batch_set_keep_bases.restype = C.c_int
        self._check(self.L.scalce_batch_set_keep_bases(self.h, int(on)))

    def exceptions_info(self, mate=0):
        """scalce_batch_exceptions_info: (entries of OUT_EXCEPTIONS, records that hold at least one) of `mate`."""
        self.L.scalce_batch_exceptions_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self.L.scalce_batch_exceptions_info.restype = C.c_int
        x, n = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.scalce_batch_exceptions_info(self.h, int(mate), C.byref(x), C.byref(n)))
        return int(x.value), int(n.value)

    def quality(self, stream=0):
        self._check(self.L.scalce_batch_quality(self.h, stream))

    def quality_plan(self, mate=0):
        """For tests: the path the last quality() took for `mate` (scalce_batch_quality_plan) -> (source, lo, A, inside);
        source 0: nothing counted, 1: tile ranges of the one-pass ingest, 2: the q' rows scanned, 3: the whole alphabet."""
        out = (C.c_uint32 * 4)()
        self._check(self.L.scalce_batch_quality_plan(self.h, int(mate), out))
        return tuple(int(x) for x in out)

    def ingest_plan(self, mate=0):
        """For tests: what the ingest of the last piece did for `mate` (scalce_batch_ingest_plan) -> (kernel, slow, line index
        built, long-name bytes); kernel 0: nothing ingested, 1: one-pass, 2: indexed out of LDS tiles, 3: indexed, direct."""
        out = (C.c_uint32 * 4)()
        self._check(self.L.scalce_batch_ingest_plan(self.h, int(mate), out))
        return tuple(int(x) for x in out)

    def tokenize(self, d_prior_counts=None, stream=0):
        self._check(self.L.scalce_batch_tokenize(self.h, d_prior_counts, stream))

    def tokenize_begin(self, stream=0):
        self._check(self.L.scalce_batch_tokenize_begin(self.h, stream))

    def tokenize_end(self, stream=0):
        self._check(self.L.scalce_batch_tokenize_end(self.h, stream))

    def set_chunks(self, starts):
        """Spill-chunk starts for the order stage instead of the -B rule; None: back to the -B rule."""
        if starts is None:
            self._check(self.L.scalce_batch_set_chunks(self.h, None, 0))
            return
        a = (C.c_uint64 * len(starts))(*[int(x) for x in starts])
        self._check(self.L.scalce_batch_set_chunks(self.h, a, len(starts)))

    def set_fused_rows(self, on=True):
        self._check(self.L.scalce_batch_set_fused_rows(self.h, int(on)))

    def chunk_plan(self, carry_in, cap, stream=0):
        """scalce_batch_chunk_plan -> (cuts, carry_out); len(cuts) == cap: the list may be cut short (see the header)."""
        cuts = np.zeros(max(1, int(cap)), dtype=np.uint64)
        n, carry = C.c_uint32(0), C.c_uint64(0)
        self._check(self.L.scalce_batch_chunk_plan(self.h, int(carry_in), cuts.ctypes.data_as(C.POINTER(C.c_uint64)), int(cap),
                                                   C.byref(n), C.byref(carry), stream))
        return cuts[: n.value].copy(), int(carry.value)

    def text_offset(self, mate, row, stream=0):
        off = C.c_uint64(0)
        self._check(self.L.scalce_batch_text_offset(self.h, int(mate), int(row), C.byref(off), stream))
        return int(off.value)

    def rewindow(self, keep_first, keep_rows, front, back, stream=0):
        """scalce_batch_rewindow; front / back = [(device ptr or None, nbytes)] per mate."""
        def arrays(pieces):
            pieces = list(pieces) + [(None, 0)] * (2 - len(pieces))
            return (C.c_void_p * 2)(*[p for p, _ in pieces]), (C.c_uint64 * 2)(*[int(n) for _, n in pieces])
        fp, fn = arrays(front)
        bp, bn = arrays(back)
        self._check(self.L.scalce_batch_rewindow(self.h, int(keep_first), int(keep_rows), fp, fn, bp, bn, stream))

    def qinput_edges(self, mate, stream=0):
        """scalce_batch_qinput_edges -> (edge[4], nsym, read_len)"""
        edge = (C.c_uint8 * 4)()
        nsym, rl = C.c_uint64(0), C.c_int32(0)
        self._check(self.L.scalce_batch_qinput_edges(self.h, int(mate), edge, C.byref(nsym), C.byref(rl), stream))
        return list(edge), int(nsym.value), int(rl.value)

    def entropy_stream(self, mate, d_table, d_symbols, nsym, stream=0):
        self._check(self.L.scalce_batch_entropy_stream(self.h, mate, d_table, d_symbols, int(nsym), stream))

    def order(self, stream=0):
        self._check(self.L.scalce_batch_order(self.h, stream))

    def emit(self, stream=0):
        self._check(self.L.scalce_batch_emit(self.h, stream))

    def entropy(self, d_table_override=None, stream=0):
        self._check(self.L.scalce_batch_entropy(self.h, d_table_override, stream))

    def entropy_begin(self, d_table_override=None, stream=0):
        """Enqueue the entropy stage and return; entropy_end / finish waits for it (several shards in flight)."""
        self._check(self.L.scalce_batch_entropy_begin(self.h, d_table_override, stream))

    def entropy_end(self, stream=0):
        self._check(self.L.scalce_batch_entropy_end(self.h, stream))

    def entropy_stream_begin(self, mate, d_table, d_symbols, nsym, stream=0):
        self._check(self.L.scalce_batch_entropy_stream_begin(self.h, mate, d_table, d_symbols, int(nsym), stream))

    def entropy_stream_prepare(self, mate, d_table, d_symbols, nsym, stream=0):
        self._check(self.L.scalce_batch_entropy_stream_prepare(self.h, mate, d_table, d_symbols, int(nsym), stream))

    def front(self, d_text1, n1, d_text2=None, n2=0, stream=0):
        """Every stage before the entropy coder (ingest .. emit) on `stream` (scalce_batch_front)."""
        self._check(self.L.scalce_batch_front(self.h, d_text1, int(n1), d_text2, int(n2), stream))

    def compress(self, d_text1, n1, d_text2=None, n2=0, stream=0):
        self._check(self.L.scalce_batch_compress(self.h, d_text1, int(n1), d_text2, int(n2), stream))

    def finish(self, stream=0):
        self._check(self.L.scalce_batch_finish(self.h, stream))

    @property
    def n_reads(self):
        return int(self.L.scalce_batch_reads(self.h))

    def output_ptr(self, which, mate=0):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.scalce_batch_output(self.h, which, mate, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def output(self, which, mate=0, dtype=np.uint8):
        p, n = self.output_ptr(which, mate)
        return self.ctx.to_host(p, n, dtype)

    def set_frame_on_demand(self, on=True):
        """The coded blocks are framed on their way out (qual_window) instead of by a copy pass behind the coder."""
        self._check(self.L.scalce_batch_set_frame_on_demand(self.h, int(on)))

    def set_code_in_place(self, on=True):
        """Grouped coder launches write a block's bytes over its own symbols (no block buffers); the caller keeps the shard's text
        in place until the shard is collected (scalce_batch_set_code_in_place)."""
        self._check(self.L.scalce_batch_set_code_in_place(self.h, int(on)))

    @property
    def reruns(self):
        self.L.scalce_batch_reruns.restype = C.c_uint64
        self.L.scalce_batch_reruns.argtypes = [C.c_void_p]
        return int(self.L.scalce_batch_reruns(self.h))

    @property
    def coder_round(self):
        """Symbols per round of the last one-block-per-lane coder launch this batch led (0: none): which kernel ran."""
        self.L.scalce_batch_coder_round.restype = C.c_int
        self.L.scalce_batch_coder_round.argtypes = [C.c_void_p]
        return int(self.L.scalce_batch_coder_round(self.h))

    def qual_bytes(self, mate=0):
        n = C.c_uint64()
        self._check(self.L.scalce_batch_qual_bytes(self.h, mate, C.byref(n)))
        return n.value

    def qual_window(self, mate, offset, nbytes, dst, stream=0):
        """bytes [offset, offset + nbytes) of SCALCE_OUT_QUAL into dst (device or pinned host pointer, 4-byte aligned)"""
        self._check(self.L.scalce_batch_qual_window(self.h, mate, int(offset), int(nbytes), dst, stream))

    def stats(self):
        a = (C.c_uint32 * 7)()
        self._check(self.L.scalce_batch_stats(self.h, a))
        return dict(tie_reads=a[0], events=a[1], jacobi_iters=a[2], chunks=a[3], order_run_members=a[4], tie_fallback=a[5],
                    order_radix_fallback=a[6])

    def tie_plan(self):
        """For tests: the path the last tie-break took (scalce_batch_tie_plan).  path 0: no tie reads, 1: windows with one
        launch per sweep, 2: windows with two launches, 3: global sweeps; window = tie reads per window as used, windows = how
        many; sequential = the counters of tie_sequential_k, 0: it did not run, 1: LDS, 2: LDS with the limit raised, 3: global
        memory."""
        a = (C.c_uint32 * 4)()
        self._check(self.L.scalce_batch_tie_plan(self.h, a))
        return dict(path=a[0], window=a[1], windows=a[2], sequential=a[3])

    def stage_reset(self, enable=True):
        self.L.scalce_batch_stage_reset(self.h, int(enable))

    def stage_ms(self):
        out = {}
        for i, name in enumerate(STAGES):
            ms, n = C.c_float(), C.c_int()
            self.L.scalce_batch_stage_ms(self.h, i, C.byref(ms), C.byref(n))
            out[name] = (ms.value, n.value)
        return out

    def kernel_timing(self, enable=True):
        self.L.scalce_batch_kernel_timing(self.h, int(enable))

    def kernel_ms(self):
        ms, n, bi, bo = C.c_double(), C.c_int(), C.c_uint64(), C.c_uint64()
        self._check(self.L.scalce_batch_kernel_ms(self.h, C.byref(ms), C.byref(n), C.byref(bi), C.byref(bo)))
        return dict(total_ms=ms.value, launches=n.value, bytes_in=bi.value, bytes_out=bo.value)

    def close(self):
        if self.h:
            self.L.scalce_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
