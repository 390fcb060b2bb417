"""Fetch-path log read on the device (rpgpu_fetch) against a plain
device-to-device copy of the same bytes.

C1-shaped data (16 KiB uncompressed batches from the seeded generator):
--parts partitions of --segs segments of --seg-mib MiB each, offsets
ascending through a partition.  Every request starts in the middle of its
partition's second segment and ends on max_bytes = half the partition, so
about half the source bytes are returned.  After the disk-layout job and
rpgpu_segment_index, rpgpu_fetch (with the entry index) and a torch copy of
bytes_out bytes are timed alternately in one process, each with HIP events on
its stream: the library's own stage events (rpgpu_set_timing) for the fetch,
torch events for the copy.  The same calls without the entry index follow, for
k_fetch_select's time alone: without the index the reader walks every batch
in front of start_offset of the segment it enters.

Prints one JSON line and writes it to --out: per-call milliseconds (median,
min, max over the alternations), GB/s of output bytes for both, their ratio,
and the fetch's per-pass milliseconds with and without the index.

    python scripts/bench_fetch.py [--parts 8] [--segs 4] [--seg-mib 8] [--steps 20] [--warmup 3] [--out profiles/fetch_bench.json]
"""
import argparse
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import synth  # noqa: E402  (test/bench data generator, not the product)
from redpanda_amd import abi  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def headers(seg: bytes):
    """(file position, base_offset, last_offset) of each whole batch."""
    out, pos = [], 0
    while len(seg) - pos >= 61:
        hcrc, size, base = struct.unpack_from("<Iiq", seg, pos)
        if hcrc == 0 or size < 61 or pos + size > len(seg):
            break
        out.append((pos, base, base + struct.unpack_from("<i", seg, pos + 23)[0]))
        pos += size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--segs", type=int, default=4)
    ap.add_argument("--seg-mib", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_bench.json"))
    a = ap.parse_args()
    import torch
    from redpanda_amd.engine import Engine
    segs, bases, start = [], [], None
    for k in range(a.segs):
        seg = np.zeros(a.seg_mib << 20, dtype=np.uint8)
        synth.gen_segment(seg, k, seed=0xC1)  # segment k's offsets start at k * 10^8
        hs = headers(seg.tobytes())
        if k == min(1, a.segs - 1):
            start = hs[len(hs) // 2][1]
        bases.append(hs[0][1])
        segs.append(seg)
    part = np.concatenate(segs)
    data = np.tile(part, a.parts)
    nseg = a.parts * a.segs
    offs = np.arange(nseg + 1, dtype=np.uint64) * np.uint64(a.seg_mib << 20)
    ps = np.arange(a.parts + 1, dtype=np.uint32) * np.uint32(a.segs)
    eng = Engine(0)
    reqs = np.array([eng.fetch_request(start, (1 << 62), part.size // 2)] * a.parts, dtype=abi.FETCH_REQUEST)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    nb, _, _ = eng.query_capacity(d, offs, abi.JOB_CRC)
    out = eng.alloc_outputs(nseg, nb + 1, 1, 1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.submit(d, offs, out, abi.JOB_CRC)
        index = eng.segment_index(out, bases * a.parts)
        stream.synchronize()
        cap = data.size + 16
        buf = torch.empty(cap, dtype=torch.uint8, device=d.device)
        bbuf = torch.empty((nb + 1) * abi.FETCH_BATCH.itemsize, dtype=torch.uint8, device=d.device)
        dst = torch.empty(cap, dtype=torch.uint8, device=d.device)
        eng.set_timing(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        runs = {}
        for name, idx in (("index", index), ("no_index", None)):
            fet, cpy, stages, tot = [], [], {}, None
            for i in range(a.warmup + a.steps):
                res = eng.fetch(d, offs, out, ps, reqs, index=idx, out_capacity=cap, out_batch_capacity=nb + 1,
                                out_buffer=buf, out_batch_buffer=bbuf, sync=False)
                t = eng.fetch_timings()  # synchronises on the call's last event
                if tot is None:
                    tot = res.totals_host()
                    assert not tot["overflow"] and int(tot["parts_ok"]) == a.parts
                n = int(tot["bytes_out"])
                e0.record(stream)
                dst[:n].copy_(buf[:n])
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    fet.append(t["total"])
                    cpy.append(e0.elapsed_time(e1))
                    for k, v in t.items():
                        stages.setdefault(k, []).append(v)
            runs[name] = (fet, cpy, stages, tot)
    fet, cpy, stages, tot = runs["index"]
    n = int(tot["bytes_out"])
    assert int(runs["no_index"][3]["bytes_out"]) == n
    fm, cm = spread(fet), spread(cpy)
    st = {k: spread(v)["median"] for k, v in stages.items()}
    line = {
        "bench": "fetch", "partitions": a.parts, "segments_per_partition": a.segs, "segment_bytes": a.seg_mib << 20,
        "input_bytes": int(data.size), "batches_in": int(out.totals_host()["n_batches"]),
        "batches_out": int(tot["batches_out"]), "bytes_out": n,
        "fetch_ms": fm, "copy_ms": cm,
        "fetch_gb_per_s": round(n / (fm["median"] * 1e-3) / 1e9, 1),
        "copy_gb_per_s": round(n / (cm["median"] * 1e-3) / 1e9, 1),
        "fetch_over_copy": round(cm["median"] / fm["median"], 3),
        "copy_pass_over_copy": round(cm["median"] / st["copy"], 3),
        "fetch_over_copy_spread": [round(c / x, 3) for c, x in sorted(zip(cpy, fet), key=lambda p: p[0] / p[1])][:: max(len(fet) - 1, 1)],
        "stage_ms": st,
        "stage_ms_no_index": {k: spread(v)["median"] for k, v in runs["no_index"][2].items()},
        "steps": a.steps, "warmup": a.warmup,
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
