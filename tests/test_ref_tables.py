"""CPU: the oracle's tokens and order pinned to the reference's own on the core-table shapes of the tokenizer tests
(tests/bigtable.py SHAPES, tests/test_gpu_tokenizer_tables.py).  Each table goes to the reference as a text list
(read_patterns_from_file: the same cores in the same file order as the patterns.bin the GPU tests load), with reads
whose cores sit at the walks' corners; oracle/_ref/ref_driver runs aho_search + aho_trie_bucket + the emission order of
aho_output on them.  With the GPU tests (device == oracle) this gives device == oracle == reference on every shape."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bigtable as B
import oraclelib as O
from scalce_amd import host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
have_ref = pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="oracle/_ref/ref_driver not built (needs the reference)")


def describe(blob, is_text):
    L = host.lib()
    L.scalce_patterns_describe_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    ns, nb = C.c_int32(), C.c_int32()
    rc = L.scalce_patterns_describe_host(blob, len(blob), int(is_text), None, 0, C.byref(ns), C.byref(nb))
    return rc, ns.value, nb.value


@pytest.mark.parametrize("name", B.SHAPES)
def test_shape_tables_load_as_built(name):
    """each table loads (binary or text) into the automaton its shape calls for: the state counts the GPU tests rely on,
    and the walk the table selects (what test_walk_of_every_shape asserts of the loaded table on the device)"""
    t = B.shape(name)
    rc, ns, nb = describe(t.blob, t.text)
    assert rc == 0
    walk = host.walk_of_table(t.blob, t.text)
    assert walk == t.walk, f"{name}: table selects {walk}, built for {t.walk}"
    assert nb == len(set(t.cores))
    if t.note.startswith("states=="):
        assert ns == int(t.note.split("==")[1]) == B.n_states(t.cores)
    elif t.note == "states>=1M":
        assert ns >= 1_000_000
    if not t.text:   # the binary table and its text form are one table
        assert describe(B.text_of(t.cores), True)[1:] == (ns, nb)
        assert host.walk_of_table(B.text_of(t.cores), True) == walk


def test_core_of_128_bases_is_refused_by_the_loader():
    assert describe(b"ACGTACGTAC\n" + b"G" * 127 + b"\n", True)[0] == 0
    assert describe(b"ACGTACGTAC\n" + b"G" * 128 + b"\n", True)[0] == 3   # SCALCE_ERR_FORMAT


@have_ref
@pytest.mark.parametrize("name", B.SHAPES)
def test_oracle_equals_reference(name, tmp_path):
    t = B.shape(name)
    (tmp_path / "p.txt").write_bytes(B.text_of(t.cores))
    trie = O.Trie(text=B.text_of(t.cores))
    for L in (32, 129):
        bases = np.concatenate([B.corner_reads(t.cores, L, 2500, seed=L + 1),
                                B.tie_reads(t.cores, L, 500, seed=L + 2) if 2 * t.min_len <= L else
                                B.corner_reads(t.cores, L, 500, seed=L + 3)])
        fq = tmp_path / f"in{L}.fq"
        fq.write_bytes(synth.fastq_bytes_fast(bases, np.full(bases.shape, ord("I"), dtype=np.uint8)))
        out = tmp_path / f"ref{L}"
        out.mkdir()
        r = subprocess.run([REF_DRIVER, str(fq), str(out), "-P", str(tmp_path / "p.txt")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        tok = np.fromfile(out / "tok.i32", dtype=np.int32).reshape(-1, 2)
        pat, end = trie.tokenize(bases)
        bad = np.flatnonzero((tok[:, 0] != pat) | (tok[:, 1] != end))
        assert len(bad) == 0, f"{name} L={L}: {len(bad)} reads differ, first {bad[:4]}"
        assert (np.fromfile(out / "order.i64", dtype=np.int64) == trie.order(bases, pat, end)).all(), f"{name} L={L}"
        assert (pat >= 0).sum() > len(bases) // 2
