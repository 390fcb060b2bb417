"""Produce-path append on the device (rpgpu_append_wire) against a plain
device-to-device copy of the same bytes.

C1-shaped data (16 KiB uncompressed batches from the seeded generator) is
serialised for the wire and tiled into --sets record sets.  After the
wire-layout job, rpgpu_append_wire (RPGPU_APPEND_ALL_BATCHES) and a torch
copy of bytes_out bytes are timed alternately in one process, each with HIP
events on its stream: the library's own stage events (rpgpu_set_timing) for
the append, torch events for the copy.

Prints one JSON line and writes it to --out: per-call milliseconds (median,
min, max over the alternations), GB/s of output bytes for both, their ratio,
and the append's per-pass milliseconds.

    python scripts/bench_append.py [--sets 8] [--set-mib 32] [--steps 20] [--warmup 3] [--out profiles/append_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import synth  # noqa: E402  (test/bench data generator, not the product)
from redpanda_amd import abi  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--set-mib", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_bench.json"))
    a = ap.parse_args()
    import torch
    from redpanda_amd.engine import Engine
    from tests import batchgen as bg
    seg = np.zeros(a.set_mib << 20, dtype=np.uint8)
    synth.gen_segment(seg, 0, seed=0xC1)
    rs = np.frombuffer(bg.disk_to_wire(seg.tobytes()), dtype=np.uint8)
    data = np.tile(rs, a.sets)
    offs = np.arange(a.sets + 1, dtype=np.uint64) * np.uint64(rs.size)
    eng = Engine(0)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    flags = abi.JOB_CRC | abi.JOB_PARSE
    nb, nr, nd = eng.query_capacity(d, offs, flags, layout=abi.LAYOUT_WIRE)
    out = eng.alloc_outputs(a.sets, nb + 1, nr + 1, 1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.submit(d, offs, out, flags, layout=abi.LAYOUT_WIRE)
        stream.synchronize()
        cap = data.size + 16
        buf = torch.empty(cap, dtype=torch.uint8, device=d.device)
        dst = torch.empty(cap, dtype=torch.uint8, device=d.device)
        nxt = [i << 32 for i in range(a.sets)]
        eng.set_timing(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        app, cpy, stages, tot = [], [], {}, None
        for i in range(a.warmup + a.steps):
            res = eng.append_wire(d, offs, out, nxt, None, True, out_capacity=cap, out_batch_capacity=nb + 1,
                                  out_buffer=buf, sync=False)
            t = eng.append_timings()  # synchronises on the call's last event
            if tot is None:
                tot = res.append_totals_host()
                assert not tot["overflow"] and int(tot["sets_ok"]) == a.sets
            n = int(tot["bytes_out"])
            e0.record(stream)
            dst[:n].copy_(buf[:n])
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                app.append(t["total"])
                cpy.append(e0.elapsed_time(e1))
                for k, v in t.items():
                    stages.setdefault(k, []).append(v)
    n = int(tot["bytes_out"])
    am, cm = spread(app), spread(cpy)
    line = {
        "bench": "append_wire", "sets": a.sets, "set_bytes": int(rs.size), "input_bytes": int(data.size),
        "batches_out": int(tot["batches_out"]), "bytes_out": n,
        "append_ms": am, "copy_ms": cm,
        "append_gb_per_s": round(n / (am["median"] * 1e-3) / 1e9, 1),
        "copy_gb_per_s": round(n / (cm["median"] * 1e-3) / 1e9, 1),
        "append_over_copy": round(cm["median"] / am["median"], 3),
        "append_over_copy_spread": [round(c / x, 3) for c, x in sorted(zip(cpy, app), key=lambda p: p[0] / p[1])][:: max(len(app) - 1, 1)],
        "stage_ms": {k: spread(v)["median"] for k, v in stages.items()},
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
