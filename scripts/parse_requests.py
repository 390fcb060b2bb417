"""Per-kernel memory-side requests of the C1 job from the PMC passes of
scripts/gpu_requests.sh -> profiles/walk_requests.json (one entry per tag, so
a before and an after stand side by side).

  python scripts/parse_requests.py TAG [bench.json]

Counters are summed over a kernel's dispatches and divided by the number of
k_chunk_base dispatches (one per submit).  TCC_EA0_RDREQ / WRREQ count the
requests L2 sends to the fabric (HBM); the _32B / _64B counters are the
requests of that size among them.  With a bench result line (bench.json:
stage_ms of an unprofiled run of the same build) the rates per second are
added: k_validate over stage_ms.validate, k_walk over stage_ms.walk."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.path.join(root, os.environ.get("OUT", "bench_out"))
dest = os.path.join(root, "profiles", "walk_requests.json")
BATCHES, RECORDS = 1048576, 16384 * 1000  # the C1 job (overridden by the bench line)
KERNELS = ("k_validate", "k_walk", "k_emit", "k_finalize_bitmap", "k_finalize_segments")


def counters(sub):
    acc = defaultdict(lambda: defaultdict(float))
    seen = defaultdict(set)
    for f in glob.glob(os.path.join(out, sub, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row.get("Kernel_Name", "").split("(")[0].replace("rp::", "").strip()
            k = k.split(" ")[-1].split("<")[0]
            acc[k][row["Counter_Name"]] += float(row["Counter_Value"])
            seen[k].add((f, row.get("Dispatch_Id")))
    return acc, {k: len(v) for k, v in seen.items()}


def main():
    tag = sys.argv[1]
    bench = None
    if len(sys.argv) > 2:
        bench = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
    batches, records = BATCHES, RECORDS
    ms = {}
    if bench:
        cfg = bench["config"]
        ms = {"k_validate": cfg["stage_ms"]["validate"], "k_walk": cfg["stage_ms"]["walk"]}
        batches, records = int(cfg["batches_per_gpu"]), int(cfg["records_per_gpu"])
    res = {"tag": tag, "batches": batches, "records": records, "kernels": {}}
    for sub in (f"pmc_req_{tag}", f"pmc_reqsplit_{tag}"):
        acc, n = counters(sub)
        subs = max(n.get("k_chunk_base", 0), 1)
        for k in KERNELS:
            if k not in acc:
                continue
            e = res["kernels"].setdefault(k, {})
            for c, v in acc[k].items():
                e[c.replace("TCC_EA0_", "").replace("_sum", "").lower()] = int(v / subs)
    for k, e in res["kernels"].items():
        if "rdreq" in e:
            tot = e["rdreq"] + e["wrreq"]
            e["requests"] = tot
            e["per_batch"] = round(tot / batches, 2)
            e["per_record"] = round(tot / records, 3)
            if k in ms:
                e["ms"] = ms[k]
                e["g_requests_per_s"] = round(tot / ms[k] / 1e6, 2)
    allres = json.load(open(dest)) if os.path.exists(dest) else {}
    allres[tag] = res
    json.dump(allres, open(dest, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
