"""rpgpu_append_wire: validated produce record sets -> the bytes the log
receives (adapt + the partition verdict + set_max_timestamp +
disk_log_appender offsets), against the CPU reference tests/append_ref.py.

The CPU part pins the reference (it does not go through the code under test)
and the ABI; the GPU part compares every output of the device with it.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from redpanda_amd import abi
from tests import append_ref as AR
from tests import batchgen as bg
import synth  # noqa: E402  (test/bench data generator, not the product)

FLAGS = abi.JOB_CRC | abi.JOB_PARSE
DFLAGS = FLAGS | abi.JOB_DECODE
MIX = (1 << abi.CODEC_NONE) | (1 << abi.CODEC_LZ4) | (1 << abi.CODEC_SNAPPY)
PIECE = 65536  # kAppendPiece (rp_internal.h): payloads are copied in pieces of this many bytes
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4097, 65535, 65536, 65537, 3 * PIECE + 17]


# ---------------------------------------------------------------------------
# record sets
# ---------------------------------------------------------------------------
def concat(sets):
    offs = np.cumsum([0] + [len(s) for s in sets]).astype(np.uint64)
    data = np.frombuffer(b"".join(bytes(s) for s in sets), dtype=np.uint8).copy()
    return data, offs


def good(n=3, seed=1, **kw):
    return AR.wire_batch(bg.simple_records(n, seed=seed), n, **kw)


def opaque(n, seed, **kw):
    """A batch of exactly n payload bytes: lz4-attributed arbitrary bytes with a
    correct crc; adapt() does not parse compressed batches."""
    pay = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    return AR.wire_batch(pay, 1, attrs=abi.CODEC_LZ4, **kw)


def junk(k):
    """61 + k bytes that are rejected: a complete batch with a wrong crc."""
    return AR.wire_batch(bytes(range(k)), 1, attrs=abi.CODEC_LZ4, crc=0x12345678)


def tiny_sets():
    return [good(1), b"", good(3, seed=2, base_offset=5) + good(2, seed=3, lod=7)]


def verdict_sets():
    """(name, set, status by default, status with ALL_BATCHES)."""
    recs = bg.simple_records(3, seed=7)
    ok, cm, ir, mf = abi.APPEND_OK, abi.APPEND_CORRUPT_MESSAGE, abi.APPEND_INVALID_RECORD, abi.APPEND_MALFORMED
    return [
        ("good", good(2, seed=4), ok, ok),
        ("bad magic", AR.wire_batch(recs, 3, magic=1), cm, cm),
        ("bad crc", AR.wire_batch(recs, 3, crc=0xDEADBEEF), cm, cm),
        ("codec 5", AR.wire_batch(recs, 3, attrs=5), mf, mf),
        ("trailing bytes", AR.wire_batch(recs + b"\x00\x00", 3), ir, ir),
        ("truncated records", AR.wire_batch(bg.simple_records(2, seed=7), 3), ir, ir),  # the third is missing
        ("good between", good(4, seed=5), ok, ok),
        ("past the end", AR.wire_batch(recs, 3)[:-5], mf, mf),
        ("batch_length too small", AR.wire_batch(recs, 3, batch_length=40), mf, mf),
        ("58 bytes", good(1)[:58], mf, mf),
        ("good then garbage", good(2, seed=6) + b"\xAB" * 100, ok, mf),
        ("good then bad crc", good(2, seed=8) + AR.wire_batch(recs, 3, crc=1), ok, cm),
        ("good last", good(1, seed=9), ok, ok),
    ]


def misaligned_sets():
    """Every length of LENGTHS as a set of its own, 16 times, each round behind
    one more rejected set of 61 + k bytes.  The rounds' k are ordered so that
    the rejected bytes so far (source minus destination position) run through
    every residue mod 16."""
    steps = [0, 1, 14, 3, 12, 5, 10, 7, 8, 9, 6, 11, 4, 13, 2, 15]  # partial sums mod 16 are all different
    ks = [(a - 61) % 16 for a in steps]
    assert sorted(ks) == list(range(16))
    sets, seed = [], 100
    for k in ks:
        sets.append(junk(k))
        for n in LENGTHS:
            sets.append(opaque(n, seed))
            seed += 1
    return sets


def bulk_sets():
    sets = []
    for i in range(64):
        seg = np.zeros(64 << 10, dtype=np.uint8)
        synth.gen_segment(seg, i, seed=0xA77, batch_bytes=0, min_batch=200, max_batch=20000, codec_mix=MIX,
                          corrupt_payload_ppm=30000 if i % 9 == 4 else 0)
        sets.append(bg.disk_to_wire(seg.tobytes()))
    big = bg.record(0, b"k", np.random.default_rng(5).integers(0, 256, (1 << 20) + 4321, dtype=np.uint8).tobytes())
    sets[17] = AR.wire_batch(big, 1) + sets[17]
    return sets


# ---------------------------------------------------------------------------
# CPU: the reference checks itself; the ABI
# ---------------------------------------------------------------------------
def reference_invariants(oracle, sets, next_offsets, append_times=None, all_batches=False, flags=FLAGS):
    data, offs = concat(sets)
    ref = AR.expected(oracle, data, offs, next_offsets, append_times, all_batches, flags)
    raw = data.tobytes()
    # the output, serialised for the wire again, is the accepted input with only base_offset rewritten
    back = bg.disk_to_wire(ref.out.tobytes())
    pos = 0
    for (s, w, size), b in zip(ref.accepted, ref.batches):
        if append_times is None or int(append_times[s]) == abi.APPEND_CREATE_TIME:
            assert back[pos + 8:pos + size] == raw[w + 8:w + size]
        else:
            assert back[pos + 61:pos + size] == raw[w + 61:w + size]
        assert struct.unpack_from(">q", back, pos)[0] == int(b["base_offset"])
        pos += size
    assert pos == len(back) == ref.out.size
    # offsets are contiguous per set, from next_offset
    for s in range(len(sets)):
        sm, st = ref.summaries[s], ref.sets[s]
        nxt = int(next_offsets[s])
        for b in ref.batches[int(sm["first_batch"]):int(sm["first_batch"]) + int(sm["n_batches"])]:
            assert int(b["base_offset"]) == nxt
            nxt = AR._i64(nxt + int(b["last_offset_delta"]) + 1)
        assert int(st["last_offset"]) == AR._i64(nxt - 1) and int(st["n_batches"]) == int(sm["n_batches"])
        assert int(sm["first_bad"]) == int(sm["n_batches"]) and int(sm["terminal_errc"]) == abi.ERRC_END_OF_STREAM
    good_flags = abi.F_HEADER_OK | abi.F_COMPLETE | abi.F_CRC_OK
    assert np.all(ref.batches["flags"] & good_flags == good_flags)
    assert not np.any(ref.batches["flags"] & abi.F_WIRE_V2)
    return ref


def test_reference_tiny_and_verdicts(oracle):
    for allb in (False, True):
        ref = reference_invariants(oracle, tiny_sets(), [0, 1 << 40, 1 << 62], None, allb)
        assert [int(x) for x in ref.sets["status"]] == [0, 0 if allb else abi.APPEND_MALFORMED, 0]
        assert [int(x) for x in ref.sets["n_batches"]] == [1, 0, 2 if allb else 1]
        cases = verdict_sets()
        ref = reference_invariants(oracle, [c[1] for c in cases], list(range(100, 100 + len(cases))), None, allb)
        assert [int(x) for x in ref.sets["status"]] == [c[3 if allb else 2] for c in cases], [c[0] for c in cases]
        by = dict(zip((c[0] for c in cases), ref.sets))
        assert int(by["good then garbage"]["first_bad"]) == 1
        assert int(by["good then bad crc"]["first_bad"]) == (1 if allb else 2)
        assert int(by["58 bytes"]["first_bad"]) == 0 and int(by["bad crc"]["first_bad"]) == 0


def test_reference_differs_from_wire_job_in_two_places(oracle):
    """A wire job and the disk job over the appended bytes report the same
    batch but for header_crc (0 on the wire) and RPGPU_F_WIRE_V2, once the
    appended offsets equal the wire's."""
    sets = [good(3, base_offset=0) + good(2, seed=2, base_offset=3)]
    data, offs = concat(sets)
    ref = AR.expected(oracle, data, offs, [0], None, True)
    src = ref.source.batches
    for f in abi.BATCH_COMPARE_FIELDS:
        if f == "header_crc":
            assert np.all(src[f] == 0) and np.array_equal(ref.batches[f], ref.batches["header_crc_computed"])
        elif f == "flags":
            np.testing.assert_array_equal(src[f], ref.batches[f] | abi.F_WIRE_V2)
        else:
            np.testing.assert_array_equal(src[f], ref.batches[f], err_msg=f)


def test_reference_set_max_timestamp_vector(oracle):
    """model/tests/record_batch_test.cc:56-80."""
    b = bg.batch(bg.simple_records(10), 10)
    crc, hcrc = b[17:21], b[0:4]
    max_ts = struct.unpack_from("<q", b, 35)[0]
    same = AR.set_max_timestamp(oracle, b, False, max_ts)
    assert same == b
    plus = AR.set_max_timestamp(oracle, b, True, max_ts + 1)
    assert plus[17:21] != crc and plus[0:4] != hcrc
    back = AR.set_max_timestamp(oracle, plus, False, max_ts)
    assert back[17:21] == crc and back[0:4] == hcrc and back == b


def test_reference_append_time(oracle):
    t = AR.TS0 + 77
    sets = [good(2), good(2, seed=2), good(2, seed=3, attrs=8, max_ts=t), opaque(500, 4)]
    ref = reference_invariants(oracle, sets, [0, 10, 20, 30], [abi.APPEND_CREATE_TIME, t, t, t])
    assert [int(x) for x in ref.batches["max_timestamp"][1:]] == [t, t, t]
    assert np.all(ref.batches["attrs"][1:] & 8) and not ref.batches["attrs"][0] & 8
    # the batch that already had bit 3 and this timestamp keeps its crc
    w = ref.accepted[2][1]
    data, _ = concat(sets)
    assert int(ref.batches["crc"][2]) == struct.unpack_from(">I", data.tobytes(), w + 17)[0]
    assert int(ref.batches["crc"][1]) != struct.unpack_from(">I", data.tobytes(), ref.accepted[1][1] + 17)[0]


def test_misaligned_sets_cover_every_offset(oracle):
    sets = misaligned_sets()
    data, offs = concat(sets)
    ref = AR.expected(oracle, data, offs, [0] * len(sets))
    seen = {}
    out_pos = 0
    for s, w, size in ref.accepted:
        seen.setdefault(size - 61, set()).add((w - out_pos) % 16)
        out_pos += size
    assert sorted(seen) == sorted(LENGTHS)
    assert all(v == set(range(16)) for v in seen.values())
    assert int(np.sum(ref.sets["status"] != 0)) == 16


def test_abi_append(rplib):
    """Fails without the feature: the entry points do not exist."""
    L = rplib.load()
    assert hasattr(L, "rpgpu_append_wire") and hasattr(L, "rpgpu_append_sizeof")
    from redpanda_amd._lib import AppendJobC
    assert [L.rpgpu_append_sizeof(i) for i in range(5)] == [
        abi.APPEND_SET.itemsize, abi.APPEND_TOTALS.itemsize, abi.BATCH_RESULT.itemsize, C.sizeof(AppendJobC), 0]
    assert L.rpgpu_append_wire(None, None, None) == abi.E_INVALID
    job = AppendJobC()
    assert L.rpgpu_append_wire(None, C.byref(job), None) == abi.E_INVALID
    assert abi.APPEND_CREATE_TIME == -(1 << 63)
    assert (abi.APPEND_OK, abi.APPEND_CORRUPT_MESSAGE, abi.APPEND_INVALID_RECORD, abi.APPEND_MALFORMED,
            abi.APPEND_SOURCE_OVERFLOW) == (0, 1, 2, 3, 4)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
GUARD = 256


def device_job(engine, data, offs, flags):
    import torch
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    total, nseg = int(offs[-1]), offs.size - 1
    out = engine.alloc_outputs(nseg, total // abi.HEADER_SIZE + nseg + 1, max(total // 4, 64),
                               max(total * 8, 1 << 16) if flags & abi.JOB_DECODE else 1)
    engine.submit(d, offs, out, flags, layout=abi.LAYOUT_WIRE)
    return d, out


def assert_parity(h, ref, guard_buf=None):
    n = int(ref.totals["bytes_out"])
    for f in abi.APPEND_TOTALS_COMPARE_FIELDS:
        assert int(h.totals[f]) == int(ref.totals[f]), f"totals.{f}"
    for f in abi.APPEND_SET_COMPARE_FIELDS:
        np.testing.assert_array_equal(h.sets[f], ref.sets[f], err_msg=f"sets.{f}")
    np.testing.assert_array_equal(h.out_seg_offsets, ref.out_seg_offsets, err_msg="out_seg_offsets")
    assert h.out.size == n
    if not np.array_equal(h.out, ref.out):
        bad = np.flatnonzero(h.out != ref.out)
        raise AssertionError(f"d_out differs at {bad.size} bytes, first {bad[:8]}")
    assert len(h.batches) == len(ref.batches)
    for f in abi.BATCH_COMPARE_FIELDS:
        np.testing.assert_array_equal(h.batches[f], ref.batches[f], err_msg=f"out_batches.{f}")
    for f in abi.APPEND_SUMMARY_COMPARE_FIELDS:
        np.testing.assert_array_equal(h.summaries[f], ref.summaries[f], err_msg=f"out_summaries.{f}")
    if guard_buf is not None:
        g = guard_buf[n:].cpu().numpy()
        assert g.size >= GUARD and np.all(g == 0xAA), "bytes past bytes_out were written"


def run_parity(engine, oracle, sets, next_offsets, append_times=None, all_batches=False, flags=FLAGS):
    import torch
    data, offs = concat(sets)
    ref = AR.expected(oracle, data, offs, next_offsets, append_times, all_batches, flags)
    d, out = device_job(engine, data, offs, flags)
    cap = int(np.sum(ref.source.batches["size_bytes"].astype(np.int64))) + 16
    buf = torch.full((cap + GUARD,), 0xAA, dtype=torch.uint8, device=d.device)
    res = engine.append_wire(d, offs, out, next_offsets, append_times, all_batches, out_capacity=cap, out_buffer=buf)
    assert_parity(res.to_host(), ref, buf)
    return res, ref, d, out, offs


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("all_batches", [False, True])
def test_gpu_tiny(engine, oracle, all_batches):
    run_parity(engine, oracle, tiny_sets(), [0, 1 << 40, 1 << 62], None, all_batches)


@gpu
def test_gpu_lengths_and_misalignment(engine, oracle):
    sets = misaligned_sets()
    run_parity(engine, oracle, sets, list(range(0, 7 * len(sets), 7)))


@gpu
@pytest.mark.parametrize("all_batches", [False, True])
def test_gpu_verdict_matrix(engine, oracle, all_batches):
    cases = verdict_sets()
    res, ref, *_ = run_parity(engine, oracle, [c[1] for c in cases], list(range(100, 100 + len(cases))), None,
                              all_batches)
    h = res.to_host()
    assert [int(x) for x in h.sets["status"]] == [c[3 if all_batches else 2] for c in cases]
    # a rejected set between two accepted ones leaves no hole
    assert int(h.totals["bytes_out"]) == int(np.sum(h.sets["bytes_out"]))
    assert np.array_equal(np.diff(h.out_seg_offsets.astype(np.int64)), h.sets["bytes_out"].astype(np.int64))


@gpu
def test_gpu_offsets(engine, oracle):
    sets = [good(2, lod=10) + good(3, seed=2) + good(1, seed=3, lod=0x7FFFFFFF),
            good(1, seed=4, lod=5) + opaque(100, 5, lod=99) + good(2, seed=6),
            good(2, seed=7, lod=41) + good(2, seed=8, lod=-1) + good(4, seed=9, lod=3)]
    res, ref, *_ = run_parity(engine, oracle, sets, [0, 1 << 40, 1 << 62], None, True)
    assert [int(x) for x in res.to_host().sets["n_batches"]] == [3, 3, 3]
    run_parity(engine, oracle, sets, [1 << 62, 0, 1 << 40], None, False)


@gpu
@pytest.mark.parametrize("all_batches", [False, True])
def test_gpu_append_time(engine, oracle, all_batches):
    t = AR.TS0 + 77
    ct = abi.APPEND_CREATE_TIME
    sets = [good(2), good(2, seed=2) + good(3, seed=12), good(2, seed=3, attrs=8, max_ts=t), opaque(5000, 4),
            good(3, seed=5), opaque(PIECE + 9, 6) + good(1, seed=13)]
    run_parity(engine, oracle, sets, [0, 10, 20, 30, 40, 50], [ct, t, t, t, ct, 12345], all_batches)
    run_parity(engine, oracle, sets, [0, 10, 20, 30, 40, 50], [ct] * 6, all_batches)


@gpu
def test_gpu_capacity(engine, oracle):
    import torch
    sets = [good(2), junk(3), opaque(4097, 1) + good(2, seed=2), good(1, seed=3)]
    nxt = [0, 5, 9, 100]
    data, offs = concat(sets)
    ref = AR.expected(oracle, data, offs, nxt, None, True)
    d, out = device_job(engine, data, offs, FLAGS)
    nbytes, nb = int(ref.totals["bytes_out"]), int(ref.totals["batches_out"])
    for cap, bcap, bits in ((nbytes + 15, nb, 1), (nbytes + 16, nb - 1, 2), (nbytes + 15, nb - 1, 3)):
        buf = torch.full((nbytes + GUARD,), 0xAA, dtype=torch.uint8, device=d.device)
        res = engine.append_wire(d, offs, out, nxt, None, True, out_capacity=cap, out_batch_capacity=bcap,
                                 out_buffer=buf, sync=False)
        torch.cuda.synchronize()
        t = res.append_totals_host()
        assert int(t["overflow"]) == bits
        assert int(t["out_capacity_needed"]) == nbytes + 16 and int(t["out_batch_capacity_needed"]) == nb
        assert int(t["bytes_out"]) == nbytes and int(t["batches_out"]) == nb
        assert np.all(buf.cpu().numpy() == 0xAA), "d_out written despite the overflow"
        assert np.all(res.batches.cpu().numpy() == 0), "d_out_batches written despite the overflow"
        np.testing.assert_array_equal(res.to_host().sets["status"], ref.sets["status"])
        # a retry at the reported sizes succeeds
        buf2 = torch.full((nbytes + 16 + GUARD,), 0xAA, dtype=torch.uint8, device=d.device)
        res = engine.append_wire(d, offs, out, nxt, None, True, out_capacity=int(t["out_capacity_needed"]),
                                 out_batch_capacity=int(t["out_batch_capacity_needed"]), out_buffer=buf2)
        assert_parity(res.to_host(), ref, buf2)
    # the engine's own retry
    res = engine.append_wire(d, offs, out, nxt, None, True, out_capacity=16, out_batch_capacity=1)
    assert_parity(res.to_host(), ref)


@pytest.fixture(scope="module")
def downstream(engine, oracle):
    sets = []
    for i in range(3):
        seg = np.zeros(96 << 10, dtype=np.uint8)
        synth.gen_segment(seg, i, seed=0xD0, batch_bytes=0, min_batch=300, max_batch=6000)
        sets.append(bg.disk_to_wire(seg.tobytes()))
    sets.insert(1, junk(7))
    nxt = [1000, 5, 1 << 33, 77]
    res, ref, d, out, offs = run_parity(engine, oracle, sets, nxt, None, True)
    return res, ref, nxt, concat(sets)[0]


@gpu
def test_gpu_downstream_segment_index(engine, oracle, downstream):
    res, ref, nxt, _ = downstream
    got = engine.index_to_host(*engine.segment_index(res, nxt, step=4096), res.n_segments)
    want = oracle.segment_index(ref.batches, ref.summaries, nxt, step=4096)
    assert sum(len(w[1]) for w in want) > 8
    for g, w in zip(got, want):
        for f in abi.INDEX_STATE.names:
            assert int(g[0][f]) == int(w[0][f]), f
        for a, b in zip(g[1:], w[1:]):
            np.testing.assert_array_equal(a, b)


@gpu
def test_gpu_downstream_serialize_wire(engine, oracle, downstream):
    res, ref, nxt, data = downstream
    wire = engine.serialize_wire(res.out, ref.out_seg_offsets, res).cpu().numpy().tobytes()
    raw = data.tobytes()
    want = b"".join(struct.pack(">q", int(b["base_offset"])) + raw[w + 8:w + size]
                    for (s, w, size), b in zip(ref.accepted, ref.batches))
    assert wire == want


@gpu
def test_gpu_downstream_validate(engine, oracle, downstream):
    res, ref, nxt, _ = downstream
    n = int(ref.totals["bytes_out"])
    got = engine.validate(res.out[:n], ref.out_seg_offsets, FLAGS)
    assert len(got.batches) == len(ref.batches)
    f = got.batches["flags"]
    ok = abi.F_HEADER_OK | abi.F_CRC_OK
    assert np.all(f & ok == ok)
    assert np.all((f & abi.F_PARSE_OK != 0) | (f & abi.F_COMPRESSED != 0))
    np.testing.assert_array_equal(got.batches["base_offset"], ref.batches["base_offset"])


@pytest.fixture(scope="module")
def bulk():
    return bulk_sets()


@gpu
@pytest.mark.parametrize("flags", [FLAGS, DFLAGS])
@pytest.mark.parametrize("all_batches", [False, True])
def test_gpu_bulk(engine, oracle, bulk, all_batches, flags):
    nxt = [i * 1000003 for i in range(len(bulk))]
    times = [abi.APPEND_CREATE_TIME if i % 5 else AR.TS0 + i for i in range(len(bulk))]
    res, ref, *_ = run_parity(engine, oracle, bulk, nxt, times, all_batches, flags)
    st = ref.sets["status"]
    assert np.any(st == 0) and (not all_batches or np.any(st != 0))
    assert int(np.max(ref.batches["size_bytes"])) > (1 << 20)
