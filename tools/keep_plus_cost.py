#!/usr/bin/env python3
"""What --keep-plus costs: the measurement behind DESIGN.md's section on the plus-line stream.

  keep_plus_cost.py gen N DIR    N records of the bench shard's shape (100 bp) with fastq-dump header lines that the third line
                                 repeats: DIR/sra_1.fq
  keep_plus_cost.py run DIR      the file through scalce_amd/bin/scalce with --keep-comments --keep-plus under -c no and -c gz:
                                 the size of PREFIX_1.scalcep (and .scalcec) beside the other three files, then -d of the archive

DIR should lie on tmpfs.  The kernel times come from `rocprofv3 --kernel-trace --stats` runs of the same two commands
(tools/prof_summary.py stats): plus_plan_k, plus_copy_k, plus_insert_plan_k, plus_insert_copy_k next to comment_plan_k,
comment_copy_k and insert_copy_k.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from scalce_amd import synth  # noqa: E402

SCALCE = os.path.join(ROOT, "scalce_amd", "bin", "scalce")
PBIN = os.path.join(ROOT, "tests", "golden", "patterns.bin")


def gen(n, d):
    os.makedirs(d, exist_ok=True)
    bases, quals = synth.reads_and_quals(n, 100, dup_frac=0.1)
    with open(os.path.join(d, "sra_1.fq"), "wb") as f:
        for r in range(n):
            h = b"SRR001666.%d 071112_SLXA-EAS1_s_7:5:1:%d:%d length=100" % (r + 1, 1 + r % 2000, 1 + (r * 7) % 2000)
            f.write(b"@" + h + b"\n" + bases[r].tobytes() + b"\n+" + h + b"\n" + quals[r].tobytes() + b"\n")
    print("sra", os.path.getsize(os.path.join(d, "sra_1.fq")), "bytes")


def once(args):
    t0 = time.perf_counter()
    r = subprocess.run([SCALCE, *args, "--patterns-bin", PBIN], capture_output=True, text=True, timeout=600)
    if r.returncode:
        sys.exit(r.stderr[-2000:])
    return time.perf_counter() - t0, r.stderr


def run(d):
    src = os.path.join(d, "sra_1.fq")
    for c in ("no", "gz"):
        dt, log = once(["-c", c, "--keep-comments", "--keep-plus", "-o", os.path.join(d, "kp_" + c), src])
        sizes = {e: os.path.getsize(os.path.join(d, "kp_%s_1.scalce%s" % (c, e))) for e in "rnqcp"}
        print("-c %s: %.2f s; r %d, n %d, q %d, c %d, p %d bytes" % (c, dt, *(sizes[e] for e in "rnqcp")))
        print("   ", *[ln.strip() for ln in log.splitlines() if "Plus lines:" in ln or "Comments:" in ln], sep="\n    ")
    dt, _ = once(["-d", "-o", os.path.join(d, "back"), os.path.join(d, "kp_no_1.scalcen")])
    print("-d: %.2f s" % dt)


if __name__ == "__main__":
    if sys.argv[1] == "gen":
        gen(int(sys.argv[2]), sys.argv[3])
    else:
        run(sys.argv[2])
