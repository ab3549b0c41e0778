#!/usr/bin/env python3
"""What --variable-length costs: inputs for the measurement in DESIGN.md section 10.

  varlen_cost.py gen N DIR    N records of the bench shard's shape (100 bp, seed of bench.py's synth) trimmed to uniform random
                              lengths in 50..100: DIR/var_1.fq, and its twin padded with N to 100: DIR/pad_1.fq
  varlen_cost.py sizes DIR    sizes of the archives DIR/var_1.scalce{r,q,l} and DIR/pad_1.scalce{r,q}

The kernel times come from rocprofv3 --kernel-trace --stats over `scalce --variable-length`, `scalce` on the padded twin and
`scalce -d` (tools/prof_summary.py stats): pad_plan_k + pad_copy_k + index_write_k per GB of input text, strip_copy_k per GB
of output text, next to index_count_k + ingest_tiles2_k.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scalce_amd import synth  # noqa: E402


def gen(n, d, L=100, lo=50):
    rng = np.random.default_rng(7)
    lens = rng.integers(lo, L + 1, size=n)
    bases, quals = synth.reads_and_quals(n, L, n_frac=0.002)
    beyond = np.arange(L)[None, :] >= lens[:, None]
    bases[beyond] = ord("N")
    quals[beyond] = 33
    pad = np.frombuffer(synth.fastq_bytes_fast(bases, quals), dtype=np.uint8)
    # the same layout as fastq_bytes_fast: drop the padded positions of both lines
    names = np.char.str_len(np.char.add("@s.", np.arange(n).astype(str))).astype(np.int64) + 1
    rec = names + 2 * (L + 1) + 2
    seq0 = np.concatenate([[0], np.cumsum(rec)])[:-1] + names
    keep = np.ones(len(pad), dtype=bool)
    rows, cols = np.nonzero(beyond)
    keep[seq0[rows] + cols] = False
    keep[seq0[rows] + cols + L + 3] = False
    os.makedirs(d, exist_ok=True)
    pad.tofile(os.path.join(d, "pad_1.fq"))
    pad[keep].tofile(os.path.join(d, "var_1.fq"))
    print("records %d, var text %d bytes, padded text %d bytes" % (n, int(keep.sum()), len(pad)))


def sizes(d):
    for stem in ("var", "pad"):
        for ext in "rql":
            p = os.path.join(d, "%s_1.scalce%s" % (stem, ext))
            if os.path.exists(p):
                print("%s_1.scalce%s %d" % (stem, ext, os.path.getsize(p)))


if __name__ == "__main__":
    if sys.argv[1] == "gen":
        gen(int(sys.argv[2]), sys.argv[3])
    else:
        sizes(sys.argv[2])
