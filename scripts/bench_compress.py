"""Write-side compressor throughput (diagnostic): rpgpu_compress_batch over
~256 MiB of mixed payloads (text / JSON / near-random, 64 KiB .. 1 MiB),
lz4 and snappy-java; wall time per call (host staging included) — the
kernel times come from a rocprofv3 kernel trace of the same run."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import compress_corpus as CC  # noqa: E402
from redpanda_amd.engine import Engine  # noqa: E402

rng = np.random.default_rng(1)
makers = [CC.text, CC.json_like, CC.mostly_random]
pays = []
tot = 0
while tot < (int(os.environ.get("MIB", "256")) << 20):
    n = int(rng.integers(65536, 1 << 20))
    pays.append(makers[len(pays) % 3](n, len(pays)))
    tot += n
e = Engine(0)
for codec in (3, 2):
    codecs = [codec] * len(pays)
    e.compress_batch(codecs[:4], pays[:4])
    t = time.perf_counter()
    res = e.compress_batch(codecs, pays)
    dt = time.perf_counter() - t
    out = sum(len(b) for _, b in res)
    assert all(s == 0 for s, _ in res)
    print(f"codec {codec}: {len(pays)} payloads {tot / 2**20:.0f} MiB -> {out / 2**20:.0f} MiB in {dt * 1e3:.1f} ms "
          f"({tot / dt / 1e9:.2f} GB/s incl. host staging)", flush=True)

# gzip: the device (rpgpu_set_device_gzip, k_deflate) against the host path
# (zlib on one core) over the same payloads in the same run, and over a set of
# small payloads (the batch sizes compaction mostly sees): wall time per call,
# host staging included on both sides, and for the device k_deflate's own time
# between HIP events on the call's stream (rpgpu_gzip_device_ms).  Then
# rpgpu_recompress over the small payloads as gzip batches, its stage times
# (rpgpu_recompress_timings) with the switch on and off; off is what the
# library did before it had the switch.  GZIP=0 skips it.
if os.environ.get("GZIP", "1") != "0":
    import json
    small = [makers[i % 3](int(rng.integers(1024, 40 << 10)), 10_000 + i) for i in range(2048)]
    rows = []
    for name, ps in (("64KiB..1MiB", pays), ("1..40KiB x2048", small)):
        nbytes = sum(len(p) for p in ps)
        codecs = [1] * len(ps)
        row = {"payloads": len(ps), "mix": name, "bytes_in": nbytes}
        for side, on in (("device", True), ("host", False)):
            e.set_device_gzip(on)
            e.set_timing(on)
            e.compress_batch(codecs[:4], ps[:4])
            before = e.gzip_device_payloads()
            t = time.perf_counter()
            res = e.compress_batch(codecs, ps)
            dt = time.perf_counter() - t
            assert all(s == 0 for s, _ in res)
            assert e.gzip_device_payloads() - before == (len(ps) if on else 0)
            row[side + "_ms"] = round(dt * 1e3, 1)
            row[side + "_GBps_in"] = round(nbytes / dt / 1e9, 4)
            row[side + "_sha"] = hash(tuple(b for _, b in res))
            if on:
                row["device_kernel_ms"] = round(e.gzip_device_ms(), 1)
                row["device_kernel_GBps_in"] = round(nbytes / (row["device_kernel_ms"] * 1e-3) / 1e9, 4)
        row["same_bytes"] = row.pop("device_sha") == row.pop("host_sha")
        rows.append(row)
        print("gzip", json.dumps(row), flush=True)
    import torch
    from tests import test_recompress as TR
    dcomp = TR.to_device(TR.laid_out(small, [1] * len(small)))
    stages = {}
    e.set_timing(True)
    for side, on in (("switch_on", True), ("switch_off", False)):
        e.set_device_gzip(on)
        for _ in range(2):  # the second run: scratch grown, code loaded
            r = e.recompress(dcomp)
            torch.cuda.synchronize()
        t = r.to_host().totals
        stages[side] = {k: round(float(v), 3) for k, v in e.recompress_timings().items()}
        stages[side]["batches_compressed"] = int(t["batches_compressed"])
        stages[side]["batches_host"] = int(t["batches_host"])
        stages[side]["bytes_out"] = int(t["bytes_out"])
        print("gzip recompress", side, json.dumps(stages[side]), flush=True)
    e.set_timing(False)
    e.set_device_gzip(False)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gzip_compress_bench.json"), "w") as f:
        json.dump({"note": "wall ms of one rpgpu_compress_batch call, staging included; same_bytes: device == this "
                           "machine's host zlib; device_kernel_ms: k_deflate between HIP events",
                   "rows": rows,
                   "recompress_note": "rpgpu_recompress over the 2048 small payloads as gzip batches, stage ms from "
                                      "rpgpu_recompress_timings; switch_off leaves them to the host, as before the switch",
                   "recompress": stages}, f, indent=1)
