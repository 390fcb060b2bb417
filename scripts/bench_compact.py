"""Key compaction on the device (rpgpu_compact): stage times and throughput.

One 2 MiB keyed segment is built in Python (128 uncompressed 16 KiB batches;
8-byte keys drawn from a set a quarter the size of the record count, so about
three of four records are superseded) and tiled into 128 segments: segments
dedupe independently, so tiling repeats the same work 128 times without
letting any key match across the copies.

Prints one JSON line: HIP-event milliseconds per stage (the mean of --steps
timed calls after --warmup), input GB/s over the whole call, and the shape.

    python scripts/bench_compact.py [--segments 128] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redpanda_amd import abi  # noqa: E402


def keyed_segment(O, seg_bytes=2 << 20, batch_bytes=16384, seed=7):
    from tests import batchgen as BG
    from tests.test_compaction import make_batch
    rnd = random.Random(seed)
    n_keys = seg_bytes // 128 // 4
    keys = [rnd.getrandbits(64).to_bytes(8, "little") for _ in range(n_keys)]
    out, size, base = [], 0, 0
    while size < seg_bytes:
        recs, n = [], 61
        while True:
            r = BG.record(len(recs), rnd.choice(keys), bytes(rnd.randrange(256) for _ in range(rnd.randrange(60, 140))))
            if n + len(r) > batch_bytes:
                break
            recs.append(r)
            n += len(r)
        b = make_batch(O, recs, base)
        if size + len(b) > seg_bytes:
            break
        out.append(b)
        size += len(b)
        base += len(recs)
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    O.build()
    seg = keyed_segment(O)
    data = np.tile(seg, a.segments)
    offs = (np.arange(a.segments + 1, dtype=np.uint64) * np.uint64(seg.size))
    eng = Engine(0)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    flags = abi.JOB_CRC | abi.JOB_PARSE | abi.JOB_DECODE
    nb, nr, nd = eng.query_capacity(d, offs, flags)
    out = eng.alloc_outputs(a.segments, nb + 1, nr + 1, nd + 64)
    eng.submit(d, offs, out, flags)
    torch.cuda.synchronize()
    eng.set_timing(True)
    acc, res = {}, None
    for i in range(a.warmup + a.steps):
        res = eng.compact(d, offs, out)
        t = eng.compact_timings()
        if i >= a.warmup:
            for k, v in t.items():
                acc[k] = acc.get(k, 0.0) + v / a.steps
    tot = res.totals_host()
    assert not tot["overflow"]
    line = {
        "bench": "compact", "segments": a.segments, "segment_bytes": int(seg.size), "input_bytes": int(data.size),
        "records_in": int(tot["records_in"]), "records_kept": int(tot["records_kept"]),
        "batches_in": int(tot["batches_in"]), "batches_out": int(tot["batches_out"]),
        "batches_rewritten": int(tot["batches_rewritten"]), "bytes_out": int(tot["bytes_out"]),
        "ms": {k: round(v, 4) for k, v in acc.items()},
        "input_gb_per_s": round(data.size / (acc["total"] * 1e-3) / 1e9, 2),
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
