"""Recompression of compacted batches: the device route (rpgpu_recompress)
against the host route it replaces, in one run.

The input is scripts/bench_compact.py's shape with LZ4 source batches: one
2 MiB keyed segment (16 KiB batches of records whose values are words from a
small vocabulary, so they compress; 8-byte keys drawn from a set a quarter
the size of the record count) tiled into --segments segments, validated and
compacted on the device once.  Then, --steps times after --warmup each:

  device route   rpgpu_recompress over rpgpu_compact's outputs where they lie
                 (HIP-event milliseconds per stage)
  host route     what a caller does without it: D2H of the compacted bytes,
                 rpgpu_compress_batch over the payloads (host pointers, staged
                 back to the device inside), the segment reassembled, H2D,
                 rpgpu_stamp (wall-clock milliseconds per step, the pointer
                 arrays built beforehand; the reassembly, a Python loop
                 here, is timed but left out of the route's throughput)

Both routes' bytes are compared once.  Prints one JSON line: the stage
milliseconds, input GB/s of each route over the compacted bytes, their ratio.

    python scripts/bench_recompress.py [--segments 128] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redpanda_amd import abi  # noqa: E402


def keyed_segment(O, codec=abi.CODEC_LZ4, seg_bytes=2 << 20, batch_bytes=16384, seed=7):
    """bench_compact.keyed_segment with compressible values and `codec` source batches
    (batch_bytes bounds the uncompressed batch)."""
    from tests import batchgen as BG
    from tests.test_compaction import make_batch
    rnd = random.Random(seed)
    n_keys = seg_bytes // 128 // 4
    keys = [rnd.getrandbits(64).to_bytes(8, "little") for _ in range(n_keys)]
    words = [bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(3, 10))) for _ in range(64)]
    out, size, base = [], 0, 0
    while size < seg_bytes:
        recs, n = [], 61
        while True:
            v = b" ".join(rnd.choice(words) for _ in range(rnd.randrange(10, 24)))
            r = BG.record(len(recs), rnd.choice(keys), v)
            if n + len(r) > batch_bytes:
                break
            recs.append(r)
            n += len(r)
        b = make_batch(O, recs, base, codec)
        if size + n > seg_bytes:
            break
        out.append(b)
        size += n
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
    L = eng.L
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    flags = abi.JOB_CRC | abi.JOB_PARSE | abi.JOB_DECODE
    nb, nr, nd = eng.query_capacity(d, offs, flags)
    out = eng.alloc_outputs(a.segments, nb + 1, nr + 1, nd + 64)
    eng.submit(d, offs, out, flags)
    comp = eng.compact(d, offs, out)
    torch.cuda.synchronize()
    ch = comp.to_host()
    in_bytes = int(ch.totals["bytes_out"])
    n = len(ch.batches)
    out_cap = 16 + sum(61 + max(int(p), int(L.rpgpu_compress_bound(int(c), int(p), 0)))
                       for p, c in zip(ch.batches["payload_len"], ch.batches["codec"]))
    obuf = torch.zeros(out_cap, dtype=torch.uint8, device="cuda")

    # device route
    eng.set_timing(True)
    acc, res = {}, None
    for i in range(a.warmup + a.steps):
        res = eng.recompress(comp, out_capacity=out_cap, out_batch_capacity=n, out_buffer=obuf)
        t = eng.recompress_timings()
        if i >= a.warmup:
            for k, v in t.items():
                acc[k] = acc.get(k, 0.0) + v / a.steps
    eng.set_timing(False)
    rh = res.to_host()
    assert not rh.totals["overflow"]

    # host route: the arrays rpgpu_compress_batch takes, built once
    host = np.zeros(in_bytes + 16, dtype=np.uint8)
    pos = ch.batches["out_pos"].astype(np.int64)
    plen = ch.batches["payload_len"].astype(np.int64)
    caps = [int(L.rpgpu_compress_bound(int(c), int(p), 0)) for c, p in zip(ch.batches["codec"], plen)]
    slot = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    frames = np.zeros(int(slot[-1]) + 16, dtype=np.uint8)
    ci = (C.c_int * n)(*[int(c) for c in ch.batches["codec"]])
    ip = (C.c_void_p * n)(*[host.ctypes.data + int(p) + 61 for p in pos])
    il = (C.c_size_t * n)(*[int(p) for p in plen])
    fr = (C.c_size_t * n)()
    op = (C.c_void_p * n)(*[frames.ctypes.data + int(s) for s in slot[:-1]])
    oc = (C.c_size_t * n)(*caps)
    ol = (C.c_size_t * n)()
    st = (C.c_int * n)()
    final = np.zeros(out_cap, dtype=np.uint8)
    dfin = torch.zeros(out_cap, dtype=torch.uint8, device="cuda")
    hacc = {}
    total = 0
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host[:in_bytes] = comp.out[:in_bytes].cpu().numpy()
        t1 = time.perf_counter()
        rc = L.rpgpu_compress_batch(eng.ctx, n, ci, ip, il, fr, op, oc, ol, st)
        assert rc == 0 and not any(st)
        t2 = time.perf_counter()
        lens = np.frombuffer(ol, dtype=np.uint64).astype(np.int64)
        npos = np.concatenate([[0], np.cumsum(61 + lens)]).astype(np.int64)
        total = int(npos[-1])
        for k in range(n):
            o = int(npos[k])
            final[o:o + 61] = host[int(pos[k]):int(pos[k]) + 61]
            final[o + 21] |= int(ci[k])
            final[o + 61:o + 61 + int(lens[k])] = frames[int(slot[k]):int(slot[k]) + int(lens[k])]
        t3 = time.perf_counter()
        dfin[:total] = torch.from_numpy(final[:total]).cuda()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        eng.stamp(dfin, npos[:-1], lens, 0, abi.STAMP_CRC)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        if i >= a.warmup:
            for k, v in (("d2h", t1 - t0), ("compress_batch", t2 - t1), ("reassemble", t3 - t2), ("h2d", t4 - t3),
                         ("stamp", t5 - t4), ("total", t5 - t0)):
                hacc[k] = hacc.get(k, 0.0) + v * 1e3 / a.steps
    same = total == rh.out.size and bool(np.array_equal(dfin[:total].cpu().numpy(), rh.out))
    dev_gbs = in_bytes / (acc["total"] * 1e-3) / 1e9
    # the reassembly is a Python loop here (a memcpy per batch in a C++ caller): left out of the route's figure
    hacc["total_without_reassemble"] = hacc["total"] - hacc["reassemble"]
    host_gbs = in_bytes / (hacc["total_without_reassemble"] * 1e-3) / 1e9
    line = {
        "bench": "recompress", "segments": a.segments, "segment_bytes": int(seg.size), "source_bytes": int(data.size),
        "input_bytes": in_bytes, "batches": n, "bytes_out": int(rh.totals["bytes_out"]),
        "batches_compressed": int(rh.totals["batches_compressed"]), "routes_agree": same,
        "device_ms": {k: round(v, 4) for k, v in acc.items()},
        "host_route_ms": {k: round(v, 4) for k, v in hacc.items()},
        "device_input_gb_per_s": round(dev_gbs, 3), "host_route_input_gb_per_s": round(host_gbs, 3),
        "device_over_host": round(dev_gbs / host_gbs, 2),
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
