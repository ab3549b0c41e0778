#!/usr/bin/env python3
"""tests/golden/exceptions_ref.npz from the REAL reference pipeline (oracle/_ref/ref_full: the reference's own compress() and
decompress()): a small input with every kind of base --keep-bases has to keep, and the text the reference's decompress() wrote
for it under -p 0 and under -p 30.  tests/test_exceptions_cpu.py holds tests/exception_ref.py against it.

    python tests/golden/make_exceptions_ref.py          (where oracle/_ref/ref_full is built)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filecases as F  # noqa: E402
from scalce_amd import synth  # noqa: E402


def generated_text(n=300, L=40, seed=20261020):
    """2 % N (half with '#', half with '!'), 5 % lower case, 1 % IUPAC letters, 1 % '!' on arbitrary bases; letters only on the
    sequence line (getval indexes its table with c - 'A')"""
    bases, quals = synth.reads_and_quals(n, L, seed=seed, dup_frac=0.1, n_frac=0.0)
    rng = np.random.default_rng(seed + 1)
    bases, quals = bases.copy(), np.maximum(quals, 35).astype(np.uint8)   # ('!' and '#' only where they are put below)
    isn = rng.random(bases.shape) < 0.02
    bases[isn] = ord("N")
    quals[isn] = np.where(rng.random(int(isn.sum())) < 0.5, ord("#"), ord("!"))
    low = (rng.random(bases.shape) < 0.05)
    bases[low] |= 0x20
    amb = np.frombuffer(b"RYKMSWBDHVUXryksw", dtype=np.uint8)
    hit = rng.random(bases.shape) < 0.01
    bases[hit] = amb[rng.integers(0, len(amb), int(hit.sum()))]
    bang = rng.random(bases.shape) < 0.01
    quals[bang] = ord("!")
    return synth.fastq_bytes_fast(bases, quals)


def reference_round_trip(text, flags, d):
    """what the reference's decompress() writes for the archive its compress() made of `text`"""
    src = os.path.join(d, "in_1.fq")
    open(src, "wb").write(text)
    tag = "p" + "_".join(flags).replace("-", "")
    out = os.path.join(d, "arc" + tag)
    subprocess.run([F.REF_FULL, "compress", F.PBIN, src, out, *flags, "-T", "1", "-t", os.path.join(d, "tmp" + tag)], check=True,
                   capture_output=True)
    back = os.path.join(d, "back" + tag)
    subprocess.run([F.REF_FULL, "decompress", F.PBIN, out + "_1.scalcen", back, "-T", "1"], check=True, capture_output=True)
    return open(back + "_1.fastq", "rb").read()


def main():
    if not os.path.exists(F.REF_FULL):
        sys.exit("oracle/_ref/ref_full missing: run `make -C oracle` where the reference's sources exist")
    text = generated_text()
    with tempfile.TemporaryDirectory() as d:
        p0 = reference_round_trip(text, [], d)
        p30 = reference_round_trip(text, ["-p", "30"], d)
    as_u8 = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    np.savez_compressed(os.path.join(HERE, "exceptions_ref.npz"), input=as_u8(text), plain_p0=as_u8(p0), plain_p30=as_u8(p30))
    print("exceptions_ref.npz:", len(text), len(p0), len(p30), "bytes of text")


if __name__ == "__main__":
    main()
