#!/usr/bin/env python3
"""What --keep-bases costs: the measurement behind DESIGN.md's section on the exception stream.

  keep_bases_cost.py gen N DIR     N records of the bench shard's shape (100 bp) in four variants: DIR/clean_1.fq (no exception at
                                   all: A C G T, no quality at the offset), DIR/n01_1.fq and DIR/n1_1.fq (0.1 % and 1 % of the
                                   bases N with '#'), DIR/lossy_1.fq (the generator's own qualities, to be run under -p 30)
  keep_bases_cost.py run DIR [K]   every variant through scalce_amd/bin/scalce from file to archive, with and without
                                   --keep-bases, alternating, K times each (default 3): wall time of the process, then the size of
                                   PREFIX_1.scalcex under -c no and -c gz beside the other three files

DIR should lie on tmpfs.  The kernel times of the count and write passes come from one `rocprofv3 --kernel-trace --stats` run of
the n1 variant with the option (tools/prof_summary.py stats): exc_count_k, exc_write_k, exc_gather_k next to index_count_k,
index_write_k and ingest_tiles2_k.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from scalce_amd import synth  # noqa: E402

SCALCE = os.path.join(ROOT, "scalce_amd", "bin", "scalce")
PBIN = os.path.join(ROOT, "tests", "golden", "patterns.bin")
VARIANTS = {"clean": [], "n01": [], "n1": [], "lossy": ["-p", "30"]}


def gen(n, d):
    os.makedirs(d, exist_ok=True)
    bases, quals = synth.reads_and_quals(n, 100, dup_frac=0.1)   # (qualities from '#' up: none at the offset)
    rng = np.random.default_rng(11)
    for name, frac in (("clean", 0.0), ("n01", 0.001), ("n1", 0.01), ("lossy", 0.0)):
        b, q = bases, quals
        if frac:
            hit = rng.random(bases.shape) < frac
            b, q = bases.copy(), quals.copy()
            b[hit], q[hit] = ord("N"), ord("#")
        with open(os.path.join(d, name + "_1.fq"), "wb") as f:
            f.write(synth.fastq_bytes_fast(b, q))
        print(name, os.path.getsize(os.path.join(d, name + "_1.fq")), "bytes")


def once(d, name, flags, out):
    t0 = time.perf_counter()
    r = subprocess.run([SCALCE, *flags, "-o", os.path.join(d, out), os.path.join(d, name + "_1.fq"), "--patterns-bin", PBIN],
                       capture_output=True, text=True, timeout=60 + os.path.getsize(os.path.join(d, name + "_1.fq")) // (20 << 20))
    dt = time.perf_counter() - t0
    if r.returncode:
        sys.exit(r.stderr[-2000:])
    return dt, r.stderr


def run(d, k):
    for name, extra in VARIANTS.items():
        times = {False: [], True: []}
        log = ""
        for _ in range(k):
            for keep in (False, True):      # alternating: both see the same drift of the machine
                dt, err = once(d, name, ["-c", "no", *extra] + (["--keep-bases"] if keep else []), name + ("_kb" if keep else "_pl"))
                times[keep].append(dt)
                log = err if keep else log
        fmt = lambda ts: " / ".join("%.2f" % t for t in ts)  # noqa: E731
        print("%s: without %s s, with --keep-bases %s s" % (name, fmt(times[False]), fmt(times[True])))
        for line in log.splitlines():
            if "Bases:" in line:
                print("   ", line.strip())
        once(d, name, ["-c", "gz", *extra, "--keep-bases"], name + "_gz")
        for stem in (name + "_kb", name + "_gz"):
            sizes = {e: os.path.getsize(os.path.join(d, "%s_1.scalce%s" % (stem, e))) for e in "rnqx"}
            print("    %s: r %d, n %d, q %d, x %d bytes (x is %.2f %% of the other three)" % (
                stem, sizes["r"], sizes["n"], sizes["q"], sizes["x"], 100.0 * sizes["x"] / (sizes["r"] + sizes["n"] + sizes["q"])))


if __name__ == "__main__":
    if sys.argv[1] == "gen":
        gen(int(sys.argv[2]), sys.argv[3])
    else:
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
