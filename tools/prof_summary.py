#!/usr/bin/env python3
"""Condense rocprofv3 output directories into the small summaries kept under profiles/.

  prof_summary.py stats <dir> <out.csv>           kernel-trace --stats run: per-kernel calls / total / avg / min / max (ms)
  prof_summary.py pmc <fetch_dir> <write_dir> <out.json> [shards]   two --pmc runs (FETCH_SIZE, WRITE_SIZE): KB per kernel
  prof_summary.py coder <dir> <out.json> <blocks>   the --pmc passes of tools/pmc_coder.sh: counters of ac_encode_lanes_k
"""
import csv, glob, json, os, sys
from collections import defaultdict


def trace_rows(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    return list(csv.DictReader(open(f[0])))


def short(name):
    return name.split("(")[0].replace("void ", "")[:60]


def stats(d, out):
    acc = defaultdict(list)
    for r in trace_rows(d):
        if "scalce::" not in r["Kernel_Name"]:
            continue
        acc[short(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    tot = sum(sum(v) for v in acc.values())
    with open(out, "w") as fo:
        w = csv.writer(fo)
        w.writerow(["kernel", "calls", "total_ms", "avg_ms", "min_ms", "max_ms", "percent"])
        for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([k, len(v), round(sum(v), 3), round(sum(v) / len(v), 4), round(min(v), 4), round(max(v), 4), round(100 * sum(v) / tot, 2)])


def counters(d, name):
    f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    acc, calls = defaultdict(float), defaultdict(int)
    for r in csv.DictReader(open(f[0])):
        if r["Counter_Name"] != name or "scalce::" not in r["Kernel_Name"]:
            continue
        acc[short(r["Kernel_Name"])] += float(r["Counter_Value"])
        calls[short(r["Kernel_Name"])] += 1
    return acc, calls


def pmc(fd, wd, out, shards=None):
    fe, calls = counters(fd, "FETCH_SIZE")
    wr, _ = counters(wd, "WRITE_SIZE")
    rows = [{"kernel": k, "calls": calls[k], "FETCH_SIZE_KB": fe[k], "WRITE_SIZE_KB": wr.get(k, 0.0)} for k in fe]
    if shards is None:  # one ingest_tiles call per shard that went through the front stages
        shards = next((r["calls"] for r in rows if "ingest_tiles" in r["kernel"]), None)
    if shards:  # shards the profiled run pushed through every stage (a coder launch may hold several)
        for r in rows:
            r["shards"] = shards
    rows.sort(key=lambda r: -(r["FETCH_SIZE_KB"] + r["WRITE_SIZE_KB"]))
    json.dump(rows, open(out, "w"), indent=1)


def coder(d, out, blocks):
    """Sums of every counter over the launches of ac_encode_lanes_k in all passes under d, per launch; instruction counts
    per symbol and per step of a workgroup (a step serves `lanes` symbols, one per block); the parked share of wave time."""
    acc, seen, kernel = defaultdict(float), defaultdict(set), None
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "ac_encode_lanes_k" not in r["Kernel_Name"]:
                continue
            kernel = short(r["Kernel_Name"])
            acc[r["Counter_Name"]] += float(r["Counter_Value"])
            seen[r["Counter_Name"]].add((f, r.get("Dispatch_Id")))
    lanes = int(os.environ.get("SCALCE_AC_LANES_USED", "28"))
    sym = blocks * 10 * 1024 * 1024
    res = {"kernel": kernel, "blocks": blocks, "lanes_per_workgroup": lanes, "symbols_per_launch": sym,
           "round": os.environ.get("SCALCE_AC_ROUND", "default")}
    for k in sorted(acc):
        res[k] = acc[k] / max(1, len(seen[k]))  # per launch
    for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS"):
        if k in res:
            res[k + "_per_symbol"] = round(res[k] / sym, 4)
            res[k + "_per_workgroup_step"] = round(res[k] / sym * lanes, 3)
    wc = res.get("SQ_WAVE_CYCLES")
    if wc:
        for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY"):
            if k in res:
                res[k + "_share_of_wave_cycles"] = round(res[k] / wc, 4)
    if res.get("SQ_WAVES") and "SQ_ACTIVE_INST_VALU" in res and wc:
        for k in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_INST_LDS"):
            if k in res:
                res[k + "_share_of_wave_cycles"] = round(res[k] / wc, 4)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if "_per_" in k or "share" in k}))


if __name__ == "__main__":
    if sys.argv[1] == "stats":
        stats(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "coder":
        coder(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        pmc(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]) if len(sys.argv) > 5 else None)
