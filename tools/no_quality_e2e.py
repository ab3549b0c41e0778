#!/usr/bin/env python3
"""File -> archive throughput of the scalce command line with and without qualities: FASTQ, the same FASTQ under -Q, and
its FASTA (-f), N reads of 100 bp (default 10 M), -c no, input and archive on tmpfs.  GB/s are bytes of FASTQ input per
second of wall time for all three, so that they compare per read.  --kernel-stats also runs each compression under
`rocprofv3 --kernel-trace --stats` and prints its longest kernels (the front stages of the one shard a CLI run is).

usage: no_quality_e2e.py [READS] [DIR] [--kernel-stats]"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scalce_amd import synth_gpu  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kernel_stats = "--kernel-stats" in sys.argv
n = int(args[0]) if args else 10_000_000
d = args[1] if len(args) > 1 else ("/dev/shm/scalce_nq" if os.path.isdir("/dev/shm") else "/tmp/scalce_nq")
os.makedirs(d, exist_ok=True)
cli = os.path.join(ROOT, "scalce_amd", "bin", "scalce")
pbin = os.path.join(ROOT, "tests", "golden", "patterns.bin")

# FASTQ made on the device; FASTA = its name lines ('@' -> '>') and sequence lines, converted in slices (one boolean
# selection over the whole text is beyond what torch indexes in one go)
text = synth_gpu.fastq_on_device(n, 100, torch.device("cuda", 0), seed=7, first_index=0)
fq, fa = os.path.join(d, "in_1.fq"), os.path.join(d, "in_1.fa")
text.cpu().numpy().tofile(fq)
with open(fa, "wb") as out:
    line0, prev_nl, SL = 0, True, 1 << 28
    for a in range(0, text.numel(), SL):
        t = text[a:a + SL]
        nl = t == 10
        line = line0 + torch.cumsum(nl, 0, dtype=torch.int64) - nl.to(torch.int64)  # line of every byte (its newline included)
        starts = torch.empty_like(nl)
        starts[0] = prev_nl
        starts[1:] = nl[:-1]
        t = torch.where(starts & ((line & 3) == 0), torch.full_like(t, ord(">")), t)
        out.write(t[(line & 3) < 2].cpu().numpy().tobytes())
        line0 = int(line[-1]) + int(nl[-1])
        prev_nl = bool(nl[-1])
del text
torch.cuda.empty_cache()
size = os.path.getsize(fq)


def compress(tag, flags, src):
    out = os.path.join(d, tag)
    cmd = [cli, *flags, "-c", "no", "-o", out, src, "--patterns-bin", pbin]
    t = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "600", *cmd], capture_output=True, text=True)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit(f"{tag}: exit {r.returncode}\n{r.stderr[-1500:]}")
    arch = sum(os.path.getsize(f) for f in glob.glob(out + "_1.scalce?"))
    elapsed = [x.strip() for x in r.stderr.splitlines() if "Time elapsed" in x]
    return dt, arch, elapsed[0] if elapsed else ""


def kernels(tag, flags, src):
    pd = os.path.join(d, "prof_" + tag)
    shutil.rmtree(pd, ignore_errors=True)
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pd, "-o", "st", "--",
           cli, *flags, "-c", "no", "-o", os.path.join(d, tag + "_prof"), src, "--patterns-bin", pbin]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{tag} under rocprofv3: exit {r.returncode}\n{r.stderr[-1500:]}")
    f = glob.glob(os.path.join(pd, "**", "*kernel_trace.csv"), recursive=True)
    acc = defaultdict(list)  # (the trace's rows, as tools/prof_summary.py reads them)
    for x in (csv.DictReader(open(f[0])) if f else []):
        if "scalce::" in x["Kernel_Name"]:
            acc[x["Kernel_Name"].split("(")[0].replace("void ", "")[:80]].append((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e6)
    tot = sum(sum(v) for v in acc.values())
    print(f"  {tag}: {tot:.2f} ms in {sum(len(v) for v in acc.values())} kernel launches")
    for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1]))[:12]:
        print(f"    {sum(v):9.3f} ms  {len(v):5d}  {k}")
    shutil.rmtree(pd, ignore_errors=True)


modes = [("fastq", [], fq), ("Q", ["-Q"], fq), ("fasta", ["-f"], fa)]
print(f"{n} reads x 100 bp: FASTQ {size / 1e9:.2f} GB, FASTA {os.path.getsize(fa) / 1e9:.2f} GB, in {d}")
for tag, flags, src in modes:
    compress(tag, flags, src)  # (warm: page cache, device init)
    dt, arch, el = compress(tag, flags, src)
    print(f"{tag:6s} {dt:6.2f} s  {size / dt / 1e9:6.2f} GB/s of FASTQ input  archive {arch / 1e6:8.1f} MB  [{el}]")
if kernel_stats:
    for tag, flags, src in modes:
        kernels(tag, flags, src)
shutil.rmtree(d, ignore_errors=True)
