"""k_walk's descriptor / verdict hand-over (k_emit -> k_walk -> k_finalize_bitmap)
against the oracle, field by field, on hand-built jobs of a few KiB.

k_walk reads a 16-byte descriptor k_emit left per batch and answers with one
8-byte verdict that k_finalize_bitmap merges into the batch result; a batch it
does not walk (incomplete, compressed, more than 256 records, a wire batch
without CRC_OK) must come through with the verdict some other kernel gave it.

Not reachable at this size: a lane's grid-stride second batch (the grid has
more lanes than any small job has batches); the full-size C1 job covers it
(bench.py's parity block).
"""
import numpy as np
import pytest

from redpanda_amd import abi

from tests import batchgen as bg
from test_gpu_parity import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = abi.JOB_CRC | abi.JOB_PARSE
OVERFLOW_RECORDS = 2  # rpgpu_job_totals.overflow bit 1: the record index did not fit


def good(n, base=0, seed=1, **kw):
    """A stored batch of n well-formed records."""
    return bg.batch(bg.simple_records(n, seed=seed, **kw), n, base_offset=base)


def recs(n, bad=None, **malformed):
    """n records; record `bad` is encoded with batchgen.record's overrides
    (length=, hdr_count=, key_len=, val_len=)."""
    out = bytearray()
    for i in range(n):
        out += bg.record(i, b"key%05d" % i, b"v" * (20 + i), **(malformed if i == bad else {}))
    return bytes(out)


def long_varint(n, bad):
    """n records; record `bad`'s length varint is replaced by a 10-byte one."""
    out = bytearray()
    for i in range(n):
        r = bg.record(i, b"key%05d" % i, b"v" * (20 + i))
        out += b"\xff" * 9 + b"\x7f" + r[1:] if i == bad else r
    return bytes(out)


def segment(batches, cut=0):
    s = b"".join(batches)
    return np.frombuffer(s[: len(s) - cut], dtype=np.uint8).copy()


def run(engine, oracle, segs, flags=FLAGS, layout=abi.LAYOUT_DISK, batch_cap=None, record_cap=None, bitmap=True,
        oracle_batch_cap=None):
    """The job on the device and in the oracle.  The device's batch and record
    buffers are larger than the capacities it is told and pre-filled, so a
    write past a capacity shows."""
    import torch
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    data = np.concatenate(segs)
    total, nseg = int(offs[-1]), len(segs)
    bc = total // abi.HEADER_SIZE + nseg + 1 if batch_cap is None else batch_cap
    rc = max(total // 4, 64) if record_cap is None else record_cap
    ref = oracle.run_job(data, offs, flags, batch_cap=oracle_batch_cap or bc, record_cap=rc, layout=layout)
    guard = 8
    out = engine.alloc_outputs(nseg, bc + guard, rc + guard, 1, bitmap=bitmap)
    whole_b, whole_r = out.batches, out.records
    whole_b[bc * abi.BATCH_RESULT.itemsize:] = 0xAB
    whole_r[rc * abi.RECORD_INDEX.itemsize:] = 0xAB
    out.batches = whole_b[: bc * abi.BATCH_RESULT.itemsize]
    out.records = whole_r[: max(rc, 1) * abi.RECORD_INDEX.itemsize]
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    engine.submit(d, offs, out, flags, layout=layout)
    torch.cuda.synchronize()
    got = out.to_host()
    assert bool((whole_b[bc * abi.BATCH_RESULT.itemsize:] == 0xAB).all()), "batch results written past batch_capacity"
    assert bool((whole_r[max(rc, 1) * abi.RECORD_INDEX.itemsize:] == 0xAB).all()), "index written past record_capacity"
    return got, ref


COUNTS = [1, 2, 3, 0, 63, 64, 65, 255, 256, 257, 3, 1, 2, 257, 1]


def test_record_counts(engine, oracle):
    """0 .. 257 records; the index bases (0, 1, 3, 6, 6, 69, 133, 198, 453,
    709, 966, 969, 970, 972, 1229) are odd for some batches and even for
    others.  257 records are walked by k_validate: k_walk marks them "not
    walked" and the merge keeps k_validate's verdict."""
    batches = [good(n, base=100 * i, seed=i + 1, vlen=12, headers=i % 2) if n else bg.batch(b"", 0, base_offset=100 * i)
               for i, n in enumerate(COUNTS)]
    got, ref = run(engine, oracle, [segment(batches)])
    assert list(ref.batches["record_count"]) == COUNTS
    assert sorted(set(int(x) & 1 for x in ref.batches["index_base"])) == [0, 1]
    assert np.all(ref.batches["flags"] & abi.F_PARSE_OK) and list(ref.batches["records_parsed"]) == COUNTS
    assert_same(got, ref)


def test_two_waves_and_a_part(engine, oracle):
    """130 batches over 2 segments: two full waves of lanes and two lanes of a third."""
    segs = [segment([good(1 + (i + s) % 5, base=10 * i, seed=1 + i % 7, vlen=8 + i % 9) for i in range(65)])
            for s in range(2)]
    got, ref = run(engine, oracle, segs)
    assert len(ref.batches) == 130 and np.all(ref.batches["flags"] & abi.F_PARSE_OK)
    assert_same(got, ref)


@pytest.mark.parametrize("shift", [0, 1])
def test_parse_failures(engine, oracle, shift):
    """Parses that stop after an odd (3) and an even (4) number of records (a
    negative header count throws there; an over-long value or key makes the
    next record's read fail), corrupted record-length varints (the reference
    parses the fields one after the other and never uses the length, so these
    still parse: they send k_walk's guess of the record's end astray),
    trailing bytes, and a record_count the payload does not hold.  `shift`
    one-record batches in front flip the parity of every index base."""
    batches = [good(1, seed=9)] * shift + [
        bg.batch(recs(7, bad=3, hdr_count=-1), 7),
        good(2),
        bg.batch(recs(7, bad=4, hdr_count=-1), 7),
        bg.batch(recs(7, bad=3, val_len=1 << 20), 7),
        bg.batch(recs(7, bad=4, key_len=1 << 20), 7),
        good(3),
        bg.batch(recs(4) + b"\x00\x01\x02", 4),      # trailing bytes
        bg.batch(recs(3), 0),                         # no records, all of it trailing
        bg.batch(recs(3), 5),                         # two records short
        bg.batch(recs(1, bad=0, hdr_count=1 << 28), 1),  # the first record already fails
        bg.batch(recs(7, bad=3, length=-5), 7),
        bg.batch(recs(6, bad=4, length=1 << 20), 6),
        bg.batch(long_varint(7, 3), 7),
        bg.batch(long_varint(7, 4), 7),
        good(5),
    ]
    got, ref = run(engine, oracle, [segment(batches)])
    rb = ref.batches[shift:]
    assert [int(x) for x in rb["records_parsed"][[0, 2, 9]]] == [3, 4, 0]
    assert [int(x) for x in rb["parse_err"][[0, 2, 9]]] == [abi.PARSE_ERR_HEADER_RESERVE] * 3
    assert not np.any(rb["flags"][[0, 2, 3, 4, 6, 7, 8, 9]] & abi.F_PARSE_OK)
    assert [int(x) for x in rb["parse_err"][[6, 7]]] == [abi.PARSE_ERR_TRAILING] * 2
    assert np.all(rb["flags"][[1, 5, 14]] & abi.F_PARSE_OK)
    assert_same(got, ref, defined_only=True)


@pytest.mark.parametrize("cap", [5, 6, 7, 8, 12])
def test_record_capacity(engine, oracle, cap):
    """Three batches of 4 records (slots 0-3, 4-7, 8-11): a capacity inside
    the second batch's slots, at a pair's boundary (6) and between the two
    entries of a pair (5, 7), at the batch's end (8), and the exact fit."""
    batches = [good(4, seed=s) for s in (1, 2, 3)]
    got, ref = run(engine, oracle, [segment(batches)], record_cap=cap)
    over = [4 * (i + 1) > cap for i in range(3)]
    assert [int(e) == abi.PARSE_ERR_INDEX_CAPACITY for e in ref.batches["parse_err"]] == over
    assert bool(int(ref.totals["overflow"]) & OVERFLOW_RECORDS) == any(over)
    assert_same(got, ref, defined_only=True)


@pytest.mark.parametrize("cap", [1, 6, 64])
def test_batch_capacity(engine, oracle, cap):
    """70 batches, room for fewer results: the verdict merge stops at the
    capacity (64: one whole bitmap word, the second wave has nothing; `run`
    checks the rows past it).  The oracle ends its scan at the capacity, so
    the summaries and totals of an overflowed job are not comparable: the
    rows, their index entries and their bitmap bits are compared with the
    first `cap` of the oracle's run with room for all."""
    batches = [good(1 + i % 3, seed=i + 1) for i in range(70)]
    got, ref = run(engine, oracle, [segment(batches)], batch_cap=cap, oracle_batch_cap=80)
    assert len(ref.batches) == 70 and len(got.batches) == cap
    assert int(got.totals["n_batches"]) == 70 and int(got.totals["overflow"]) & 1
    for f in abi.BATCH_COMPARE_FIELDS:
        np.testing.assert_array_equal(got.batches[f], ref.batches[f][:cap], err_msg=f"batches.{f}")
    nr = int(ref.batches["index_base"][cap - 1] + ref.batches["records_parsed"][cap - 1])
    assert len(got.records) == nr
    for f in abi.RECORD_COMPARE_FIELDS:
        np.testing.assert_array_equal(got.records[f], ref.records[f][:nr], err_msg=f"records.{f}")
    gb = np.unpackbits(got.bitmap.view(np.uint8), bitorder="little")[:cap]
    rb = np.unpackbits(ref.bitmap.view(np.uint8), bitorder="little")[:cap]
    np.testing.assert_array_equal(gb, rb, err_msg="valid bitmap")


def test_incomplete_last_batch(engine, oracle):
    got, ref = run(engine, oracle, [segment([good(3), good(2, seed=2), good(4, seed=3)], cut=10), segment([good(2)])])
    assert not int(ref.batches["flags"][2]) & abi.F_COMPLETE
    assert_same(got, ref)


def test_compressed_without_decode(engine, oracle):
    """Compressed batches in a job without DECODE are not walked at all."""
    lz4 = bg.batch(b"\x04\x22\x4d\x18" + bytes(range(40)), 3, attrs=abi.CODEC_LZ4)
    snappy = bg.batch(bytes(range(50)), 2, attrs=abi.CODEC_SNAPPY)
    got, ref = run(engine, oracle, [segment([good(2), lz4, good(3, seed=2), snappy, good(1, seed=3)])])
    assert not np.any(ref.batches["flags"][[1, 3]] & abi.F_PARSED)
    assert_same(got, ref)


def test_parse_without_bitmap(engine, oracle):
    """No bitmap output: the verdicts still reach the batch results."""
    batches = [good(3), bg.batch(recs(5, bad=2, hdr_count=-1), 5), good(257, seed=4, vlen=4, headers=0), good(2, seed=5)]
    got, ref = run(engine, oracle, [segment(batches)], bitmap=False)
    assert got.bitmap is None and np.all(ref.batches["flags"] & abi.F_PARSED)
    assert_same(got, ref, defined_only=True)


def test_wire_layout(engine, oracle):
    """Record sets: a batch with a bad crc is not walked (its flags are the
    CRC kernel's alone), a batch whose records fail to parse is the first one
    rejected."""
    bad_crc = bg.batch(recs(3), 3, crc=0x12345678)
    bad_rec = bg.batch(recs(5, bad=2, hdr_count=-1), 5)
    sets = [
        [good(2), good(3, seed=2), bad_rec, good(1, seed=3), bad_crc, good(2, seed=4)],
        [good(4), bad_crc, good(2, seed=2), bad_rec],
        [good(1), good(2, seed=2)],
    ]
    segs = [np.frombuffer(bg.disk_to_wire(b"".join(s)), dtype=np.uint8).copy() for s in sets]
    got, ref = run(engine, oracle, segs, layout=abi.LAYOUT_WIRE)
    assert [int(x) for x in ref.summaries["first_bad"]] == [2, 1, 2]
    assert_same(got, ref, defined_only=True)
