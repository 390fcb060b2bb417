"""Key compaction of segments (rpgpu_compact).

CPU tests pin the Python reference (tests/compaction_ref.py) against the
reference's own vector (storage/tests/compaction_index_format_tests.cc:153-195)
and a batch whose expected bytes are built by hand with tests/batchgen.py, and
check the ABI.  GPU tests compare the device with that reference bit for bit:
keep bitmap, output bytes, segment offsets, batch / segment entries and totals,
and run the device's output back through the validator.
"""
import ctypes as C
import random

import numpy as np
import pytest

from redpanda_amd import abi
from tests import batchgen as BG
from tests import compaction_ref as CR

DFLAGS = abi.JOB_CRC | abi.JOB_PARSE | abi.JOB_DECODE
GOOD = abi.F_HEADER_OK | abi.F_CRC_OK | abi.F_PARSE_OK
TS0 = 1600000000000


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def make_batch(O, records, base, codec=0, attrs=0, first_ts=TS0):
    """A disk batch of the given encoded records (codec 2 / 3: compressed with
    oracle.compress); the payload crc comes from the oracle's C crc32c."""
    payload = b"".join(records)
    n = len(records)
    if codec:
        payload = O.compress(codec, payload)
    a = attrs | codec
    crc = O.crc32c(payload, O.crc32c(BG.be_prefix(a, n - 1, first_ts, first_ts + max(n - 1, 0), -1, -1, -1, n)))
    return BG.batch(payload, n, base_offset=base, attrs=a, first_ts=first_ts, crc=crc)


def keyed_batch(O, keys, base, codec=0, attrs=0, vlen=12, ts_step=1, first_ts=TS0, seed=0):
    rnd = random.Random(seed)
    recs = [BG.record(i, k, bytes(rnd.randrange(256) for _ in range(vlen)), ts_delta=i * ts_step)
            for i, k in enumerate(keys)]
    return make_batch(O, recs, base, codec, attrs, first_ts)


def as_seg(batches):
    return np.frombuffer(b"".join(batches), dtype=np.uint8).copy()


def tiny_segment(O):
    """3 uncompressed batches of 4 records: the first is fully superseded by
    the third, the second fully kept, the third partly kept (its first `a`
    is superseded by its last)."""
    return as_seg([keyed_batch(O, [b"a", b"b", b"a", b"b"], 0, seed=1),
                   keyed_batch(O, [b"e", b"f", b"g", b"h"], 4, seed=2),
                   keyed_batch(O, [b"a", b"b", b"c", b"a"], 8, seed=3)])


def key_set():
    """32 keys: null, empty (the same key), and lengths 1, 7, 8, 9, 255 and 4096."""
    rnd = random.Random(5)
    keys = [None, b""]
    for i, n in enumerate([1, 7, 8, 9, 255] * 5 + [4096, 1, 7, 4096, 8]):
        keys.append(bytes([i]) if n == 1 else bytes(rnd.randrange(256) for _ in range(n - 1)) + bytes([i]))
    assert len(keys) == 32 and len(set(k or b"" for k in keys)) == 31
    return keys


def bulk_segment(O, keys, codecs, n_batches, base, seed):
    """Batches of 1..130 records over keys[:26] (so most are fully
    superseded), then per codec a partly kept and a fully kept batch over
    the six keys the bulk never uses."""
    rnd = random.Random(seed)
    out, off = [], base

    def add(ks, codec):
        nonlocal off
        recs = []
        for i, k in enumerate(ks):
            v = bytes(rnd.randrange(256) for _ in range(rnd.randrange(301)))
            hs = [(bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(1, 6))),
                   bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 9)))) for _ in range(rnd.randrange(4))]
            recs.append(BG.record(i, k, v if rnd.randrange(8) else None, hs))
        out.append(make_batch(O, recs, off, codec))
        off += len(ks)

    for _ in range(n_batches):
        add([keys[rnd.randrange(26)] for _ in range(rnd.choice([1, 2, 63, 64, 65, 130]))], rnd.choice(codecs))
    tail = keys[26:]
    for i, c in enumerate(codecs):
        add([tail[2 * i], keys[0]], c)   # partly kept: keys[0] comes again below
        add([tail[2 * i + 1]], c)        # fully kept
    add([keys[0]], codecs[0])
    return as_seg(out)


def mixed_segments(O):
    keys = key_set()
    s0 = bulk_segment(O, keys, [abi.CODEC_NONE], 85, 0, seed=11)
    s1 = bulk_segment(O, keys, [abi.CODEC_LZ4, abi.CODEC_SNAPPY], 85, 100000, seed=12)
    s2 = bulk_segment(O, keys, [abi.CODEC_NONE], 16, 200000, seed=13)
    # one payload byte of the third batch flipped: its crc fails
    pos = 0
    for _ in range(2):
        pos += int(np.frombuffer(s2[pos + 4:pos + 8].tobytes(), dtype="<i4")[0])
    s2[pos + 61 + 3] ^= 0x40
    return [s0, s1, s2]


def ovint(v, extra):
    """vint(v) padded with `extra` redundant continuation bytes."""
    b = bytearray(BG.vint(v))
    for _ in range(extra):
        b[-1] |= 0x80
        b.append(0)
    return bytes(b)


def quirk_record(i, key, value, headers=(), pad=1, ts=None):
    """A record whose varints all carry `pad` redundant bytes."""
    body = bytearray([0])
    body += ovint(i if ts is None else ts, pad) + ovint(i, pad)
    body += ovint(len(key), pad) + key + ovint(len(value), pad) + value
    body += ovint(len(headers), pad)
    for hk, hv in headers:
        body += ovint(len(hk), pad) + hk + ovint(len(hv), pad) + hv
    return ovint(len(body), pad) + bytes(body)


def quirk_segments(O):
    """[(name, segment, expected status)]; cases the oracle's walk rejects are dropped."""
    hs = [(b"hk", b"hv"), (b"x", b"")]
    over = [make_batch(O, [quirk_record(i, k, b"v%d" % i, hs, pad=1 + i % 3) for i, k in enumerate([b"a", b"b", b"a", b"c"])], 0),
            make_batch(O, [quirk_record(i, k, b"w%d" % i, hs[:1], pad=2) for i, k in enumerate([b"d", b"e"])], 4)]
    times = [keyed_batch(O, [b"x", b"y", b"x"], 0, attrs=8, ts_step=10),
             keyed_batch(O, [b"p", b"q", b"p"], 3, attrs=0, ts_step=10)]
    long_a = bytes(range(256)) * 273 + b"A" * 112
    long_b = long_a[:65515] + b"B" * (70000 - 65515)
    assert len(long_a) == len(long_b) == 70000 and long_a[:65515] == long_b[:65515] and long_a != long_b
    longk = [keyed_batch(O, [long_a, b"s", long_b], 0)]
    repeat = [keyed_batch(O, [b"a", b"b"], 0), keyed_batch(O, [b"c", b"d"], 1)]
    # records that end with their payload: a header count of 3 with one header stored (the
    # parser keeps two empty ones, the rewrite writes them), a value cut off after 4 of 10 bytes
    cut = [make_batch(O, [BG.record(0, b"m", b"1"), BG.record(1, b"n", b"2"),
                          BG.record(2, b"m", b"3", [(b"hk", b"hv")], hdr_count=3)], 0),
           make_batch(O, [BG.record(0, b"o", b"1"), BG.record(1, b"p", b"2"),
                          BG.record(2, b"o", b"abcd", val_len=10)[:-1]], 3)]
    cases = [("overlong", over, abi.COMPACT_OK), ("timestamps", times, abi.COMPACT_OK),
             ("long_keys", longk, abi.COMPACT_OK), ("offsets", repeat, abi.COMPACT_OFFSETS),
             ("cut_short", cut, abi.COMPACT_OK)]
    kept = []
    for name, batches, status in cases:
        ok = True
        for b in batches:
            rc = int(np.frombuffer(b[57:61], dtype="<i4")[0])
            n, perr, trailing, _ = O.walk_records(b[61:], rc)
            ok &= n == rc and perr == 0 and trailing == 0
        if ok:
            kept.append((name, as_seg(batches), status))
    assert [k[0] for k in kept[:3]] == ["overlong", "timestamps", "long_keys"]
    return kept


# ---------------------------------------------------------------------------
# CPU: the reference module, pinned independently of itself
# ---------------------------------------------------------------------------
def _ref_compact(O, segs):
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    data = np.concatenate(segs)
    job = O.run_job(data, offs, DFLAGS)
    return CR.compact(data, offs, job), job, data, offs


def test_reference_vector_two_alternating_keys(oracle):
    """compaction_index_format_tests.cc:153-195 (key_reducer_max_mem): 100
    entries over two alternating 1 KiB keys at offsets 0..99 -> {98, 99}."""
    k1, k2 = b"\x01" * 1024, b"\x02" * 1024
    batches = [keyed_batch(oracle, [k1 if (b * 10 + i) % 2 == 0 else k2 for i in range(10)], b * 10, seed=b)
               for b in range(10)]
    ref, job, _, _ = _ref_compact(oracle, [as_seg(batches)])
    assert ref.segments[0]["status"] == abi.COMPACT_OK
    assert ref.kept_offsets[0] == [98, 99]
    bits = [i for i in range(len(job.records)) if (int(ref.keep[i >> 6]) >> (i & 63)) & 1]
    assert bits == [98, 99]
    assert int(ref.totals["records_in"]) == 100 and int(ref.totals["records_kept"]) == 2


def test_hand_built_partly_kept_batch(oracle):
    """One batch, keys a, b, a, c: the expected bytes are built here with
    batchgen, not with the reference module."""
    vals = [b"v0", b"v1", b"v2", b"v3"]
    recs = [BG.record(i, k, v) for i, (k, v) in enumerate(zip([b"a", b"b", b"a", b"c"], vals))]
    seg = np.frombuffer(BG.batch(b"".join(recs), 4, base_offset=7, first_ts=TS0), dtype=np.uint8)
    ref, _, _, _ = _ref_compact(oracle, [seg])
    payload = b"".join(recs[1:])
    body = BG.HDR.pack(0, 61 + len(payload), 7, 1, 0, 0, 3, TS0 + 1, (TS0 + 1) + 3, -1, -1, -1, 3)
    crc = BG.crc32c(payload, BG.crc32c(BG.be_prefix(0, 3, TS0 + 1, TS0 + 4, -1, -1, -1, 3)))
    body = body[:17] + crc.to_bytes(4, "little") + body[21:]
    want = BG.crc32c(body[4:]).to_bytes(4, "little") + body[4:] + payload
    assert ref.out.tobytes() == want
    assert ref.kept_offsets[0] == [8, 9, 10]
    e = ref.batches[0]
    assert (int(e["kept"]), int(e["flags"]), int(e["payload_len"])) == (3, abi.COMPACT_F_REWRITTEN, len(payload))


def test_reference_reencodes_overlong_varints(oracle):
    """The rewrite is canonical (shorter) and keeps the parsed length field."""
    segs = quirk_segments(oracle)
    ref, job, data, offs = _ref_compact(oracle, [segs[0][1]])
    e = ref.batches[0]
    assert int(e["flags"]) == abi.COMPACT_F_REWRITTEN and int(e["kept"]) == 3
    canon = b"".join(CR.reencode(CR.payload_of(data, offs, job, job.batches[0]), job.records[i]) for i in (1, 2, 3))
    assert ref.out[61:61 + int(e["payload_len"])].tobytes() == canon
    stored = int(job.records[3]["end_pos"]) - int(job.records[1]["rec_pos"])
    assert len(canon) < stored
    # the length field is the parsed one: stale, larger than the re-encoded body
    first = CR.reencode(CR.payload_of(data, offs, job, job.batches[0]), job.records[1])
    v, br = CR.vint_read(first, 0)
    assert v == int(job.records[1]["length"]) and br == 1 and v > len(first) - br
    # the fully kept batch stays verbatim, over-long varints included
    e1 = ref.batches[1]
    assert int(e1["flags"]) == 0
    p1 = int(e1["out_pos"]) + 61
    assert ref.out[p1:p1 + int(e1["payload_len"])].tobytes() == CR.payload_of(data, offs, job, job.batches[1])


def test_reference_records_cut_short_by_their_payload(oracle):
    """parse_record_headers keeps an (empty) header for every one the count
    announces, and fields missing at the end of the payload read as zero:
    append_record_to_buffer writes them all.  Expected bytes built by hand."""
    cases = {c[0]: c[1] for c in quirk_segments(oracle)}
    assert "cut_short" in cases, "the oracle's walk accepts both records"
    ref, _, _, _ = _ref_compact(oracle, [cases["cut_short"]])
    assert [int(e["flags"]) for e in ref.batches] == [abi.COMPACT_F_REWRITTEN] * 2
    want = [BG.record(1, b"n", b"2") + BG.record(2, b"m", b"3", [(b"hk", b"hv")], hdr_count=3) + b"\0\0" * 2,
            BG.record(1, b"p", b"2") + BG.record(2, b"o", b"abcd", val_len=10)[:-1] + b"\0"]
    for e, w in zip(ref.batches, want):
        p = int(e["out_pos"]) + 61
        assert ref.out[p:p + int(e["payload_len"])].tobytes() == w


def test_abi_exports_and_sizes(rplib):
    L = rplib.load()
    assert hasattr(L, "rpgpu_compact")
    assert [L.rpgpu_compact_sizeof(i) for i in range(4)] == [
        abi.COMPACT_BATCH.itemsize, abi.COMPACT_SEGMENT.itemsize, abi.COMPACT_TOTALS.itemsize,
        C.sizeof(rplib.CompactJobC)]
    assert L.rpgpu_compact(None, None, None) == abi.E_INVALID


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def run_device(engine, O, segs, **kw):
    """(device HostCompactResult, reference RefCompact, oracle job, device CompactResult)."""
    import torch
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    data = np.concatenate(segs)
    job = O.run_job(data, offs, DFLAGS)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    out = engine.alloc_outputs(len(segs), len(job.batches) + 3, len(job.records) + 5,
                               int(job.totals["decoded_bytes"]) + 64)
    engine.submit(d, offs, out, DFLAGS)
    dev = engine.compact(d, offs, out, **kw)
    torch.cuda.synchronize()
    return dev.to_host(), CR.compact(data, offs, job), job, dev


def assert_parity(got, ref):
    np.testing.assert_array_equal(got.keep, ref.keep, err_msg="keep bitmap")
    np.testing.assert_array_equal(got.out_seg_offsets, ref.out_seg_offsets, err_msg="out_seg_offsets")
    for f in abi.COMPACT_SEGMENT_COMPARE_FIELDS:
        np.testing.assert_array_equal(got.segments[f], ref.segments[f], err_msg=f"segments.{f}")
    for f in abi.COMPACT_TOTALS_COMPARE_FIELDS:
        assert int(got.totals[f]) == int(ref.totals[f]), f"totals.{f}"
    assert len(got.batches) == len(ref.batches)
    for f in abi.COMPACT_BATCH_COMPARE_FIELDS:
        np.testing.assert_array_equal(got.batches[f], ref.batches[f], err_msg=f"batches.{f}")
    assert got.out.size == ref.out.size
    bad = np.nonzero(got.out != ref.out)[0]
    assert bad.size == 0, f"output bytes differ first at {bad[:8]}"


def assert_output_validates(engine, got):
    import torch
    if got.out.size == 0:
        return
    d = torch.from_numpy(np.concatenate([got.out, np.zeros(16, np.uint8)])).cuda()[: got.out.size]
    v = engine.validate(d, got.out_seg_offsets, abi.JOB_CRC | abi.JOB_PARSE)
    assert len(v.batches) == len(got.batches)
    assert np.all((v.batches["flags"] & GOOD) == GOOD)
    np.testing.assert_array_equal(v.batches["record_count"].astype(np.uint32), got.batches["kept"])


def outcomes(ref, job):
    """per codec: (dropped, passed through, rewritten) source batches of OK segments"""
    out = {}
    used = {int(e["src_batch"]): int(e["flags"]) for e in ref.batches}
    for s, g in enumerate(ref.segments):
        if g["status"] != abi.COMPACT_OK:
            continue
        fb, nb = int(job.summaries[s]["first_batch"]), int(job.summaries[s]["n_batches"])
        for b in range(fb, fb + nb):
            o = out.setdefault(int(job.batches[b]["attrs"]) & 7, [0, 0, 0])
            o[0 if b not in used else 2 if used[b] & abi.COMPACT_F_REWRITTEN else 1] += 1
    return out


@pytest.mark.gpu
def test_gpu_tiny(engine, oracle):
    got, ref, job, _ = run_device(engine, oracle, [tiny_segment(oracle)])
    assert outcomes(ref, job) == {abi.CODEC_NONE: [1, 1, 1]}
    assert_parity(got, ref)
    assert_output_validates(engine, got)


@pytest.mark.gpu
def test_gpu_mixed(engine, oracle):
    got, ref, job, _ = run_device(engine, oracle, mixed_segments(oracle))
    assert [int(s) for s in ref.segments["status"]] == [abi.COMPACT_OK, abi.COMPACT_OK, abi.COMPACT_NOT_CLEAN]
    oc = outcomes(ref, job)
    assert sorted(oc) == [abi.CODEC_NONE, abi.CODEC_SNAPPY, abi.CODEC_LZ4]
    assert all(min(v) >= 1 for v in oc.values()), oc
    assert_parity(got, ref)
    # no keep bit and no output for the segment that is not clean
    ib = int(job.batches[int(job.summaries[2]["first_batch"])]["index_base"])
    assert not any((int(got.keep[i >> 6]) >> (i & 63)) & 1 for i in range(ib, len(job.records)))
    assert int(got.out_seg_offsets[2]) == int(got.out_seg_offsets[3])
    # a compressed batch passed through carries decoded_crc
    n = 0
    for e in got.batches:
        src = job.batches[int(e["src_batch"])]
        if int(e["codec"]) and not int(e["flags"]):
            p = int(e["out_pos"])
            hdr = got.out[p:p + 61].tobytes()
            assert int.from_bytes(hdr[17:21], "little") == int(src["decoded_crc"])
            assert int.from_bytes(hdr[0:4], "little") == int(src["decoded_header_crc"])
            assert int.from_bytes(hdr[21:23], "little") & 7 == 0
            n += 1
    assert n >= 2
    assert_output_validates(engine, got)


@pytest.mark.gpu
def test_gpu_quirks(engine, oracle):
    cases = quirk_segments(oracle)
    got, ref, job, _ = run_device(engine, oracle, [c[1] for c in cases])
    assert [int(s) for s in ref.segments["status"]] == [c[2] for c in cases]
    # the over-long segment: one batch rewritten (shorter than stored), one verbatim
    assert [int(e["flags"]) for e in ref.batches[:2]] == [abi.COMPACT_F_REWRITTEN, 0]
    # the 70,000-byte keys are one key: the first is dropped
    names = [c[0] for c in cases]
    s = names.index("long_keys")
    assert int(ref.segments[s]["records_in"]) == 3 and int(ref.segments[s]["records_kept"]) == 2
    # log append time keeps max_timestamp, create time takes first + last delta
    t = names.index("timestamps")
    e0, e1 = [e for e in ref.batches if int(job.batches[int(e["src_batch"])]["segment"]) == t]
    h0 = ref.out[int(e0["out_pos"]):int(e0["out_pos"]) + 61].tobytes()
    h1 = ref.out[int(e1["out_pos"]):int(e1["out_pos"]) + 61].tobytes()
    assert BG.HDR.unpack(h0)[7:9] == (TS0 + 10, TS0 + 2) and BG.HDR.unpack(h1)[7:9] == (TS0 + 10, TS0 + 10 + 20)
    assert_parity(got, ref)
    assert_output_validates(engine, got)


@pytest.mark.gpu
def test_gpu_capacity_one_byte_short(engine, oracle):
    import torch
    segs = [tiny_segment(oracle)]
    _, ref, _, _ = run_device(engine, oracle, segs)
    need = int(ref.totals["out_capacity_needed"])
    buf = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    got, _, _, _ = run_device(engine, oracle, segs, out_buffer=buf, out_capacity=need - 1, sync=False)
    assert int(got.totals["overflow"]) & 1
    assert int(got.totals["out_capacity_needed"]) == need
    assert int(got.totals["out_batch_capacity_needed"]) == len(ref.batches)
    assert bool(torch.all(buf == 0xA5)), "bytes written although the capacity was too small"
    # exactly enough: succeeds, and the guard after the buffer stays
    got, _, _, _ = run_device(engine, oracle, segs, out_buffer=buf, out_capacity=need, sync=False)
    assert int(got.totals["overflow"]) == 0
    assert_parity(got, ref)
    assert bool(torch.all(buf[need:] == 0xA5))
    # and the wrapper's retry gets there on its own
    got, _, _, _ = run_device(engine, oracle, segs, out_capacity=need - 1, out_batch_capacity=1)
    assert_parity(got, ref)


@pytest.mark.gpu
def test_gpu_table_load(engine, oracle):
    """20,000 records over 16,384 distinct 4-byte keys: the table at its
    fullest (32,768 words hold 16,384 keys); keep bitmap only."""
    rnd = random.Random(3)
    ids = list(range(16384)) + [rnd.randrange(16384) for _ in range(20000 - 16384)]
    rnd.shuffle(ids)
    batches = [make_batch(oracle, [BG.record(i, k.to_bytes(4, "little"), b"") for i, k in enumerate(ids[o:o + 100])], o)
               for o in range(0, 20000, 100)]
    got, ref, job, _ = run_device(engine, oracle, [as_seg(batches)])
    assert len(job.records) == 20000 and int(ref.totals["records_kept"]) == 16384
    np.testing.assert_array_equal(got.keep, ref.keep)
