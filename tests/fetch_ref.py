"""CPU model of rpgpu_fetch: the read rule of include/rpgpu.h ("The read,
exactly"), one batch at a time, from pieces that already exist:

  source     the oracle's disk-layout job (oracle.run_job)
  entries    oracle.segment_index (segment_index::maybe_track), looked up as
             segment_index::find_nearest does (storage/segment_index.cc:95-120)
  read       storage::log_reader + skipping_consumer (storage/log_reader.cc:
             26-119, :212-343) over a log_reader_config
  output     oracle.serialize_wire (kafka::writer_serialize_batch) over the
             returned batches

tests/test_fetch.py checks this module against the reference's own reader
tests before the GPU tests compare the device with it.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from redpanda_amd import abi
from tests import batchgen as bg

M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
TS0 = 1600000000000
NO_LIMIT = M64


def _i64(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def disk_batch(oracle, payload: bytes, record_count: int, **kw) -> bytes:
    """bg.batch with the payload crc from the oracle's C loop (bg.crc32c is a
    Python loop; the large payloads of the copy tests would take seconds)."""
    if "crc" not in kw:
        lod = kw.get("lod")
        lod = record_count - 1 if lod is None else lod
        first_ts = kw.get("first_ts", TS0)
        prefix = bg.be_prefix(kw.get("attrs", 0), lod, first_ts, first_ts + max(record_count - 1, 0), kw.get("pid", -1),
                              kw.get("epoch", -1), kw.get("seq", -1), record_count)
        kw["crc"] = oracle.crc32c(payload, oracle.crc32c(prefix))
    return bg.batch(payload, record_count, **kw)


def request(start_offset: int, max_offset: int, max_bytes: int = NO_LIMIT, strict: bool = False, type_filter=None,
            first_timestamp=None):
    """One abi.FETCH_REQUEST row (a storage::log_reader_config)."""
    flags = (abi.FETCH_STRICT_MAX_BYTES if strict else 0) | (abi.FETCH_TYPE_FILTER if type_filter is not None else 0)
    flags |= abi.FETCH_FIRST_TIMESTAMP if first_timestamp is not None else 0
    return (start_offset, max_offset, max_bytes, first_timestamp or 0, flags, type_filter or 0, (0, 0, 0))


def requests(rows) -> np.ndarray:
    return np.array(list(rows), dtype=abi.FETCH_REQUEST)


def lower_bound(a, needle) -> int:
    """std::lower_bound as libstdc++ writes it (the index arrays ascend in
    every real segment; this pins the answer where they do not)."""
    lo, n = 0, len(a)
    while n:
        half = n >> 1
        if int(a[lo + half]) < needle:
            lo += half + 1
            n -= half + 1
        else:
            n = half
    return lo


def find_nearest(entry, start: int):
    """segment_index::find_nearest(model::offset): the entry's file position, or None."""
    state, rel, _, pos = entry
    if start < int(state["base_offset"]) or len(rel) == 0:
        return None
    needle = (start - int(state["base_offset"])) & 0xFFFFFFFF
    i = lower_bound(rel, needle)
    if i == len(rel):
        i -= 1
    while True:
        if int(rel[i]) <= needle:
            return int(pos[i])
        if i == 0:
            return None
        i -= 1


def chain_of(src, s: int):
    """Job-wide ordinals of segment s's chain: its complete batches."""
    sm = src.summaries[s]
    first, n = int(sm["first_batch"]), int(sm["n_batches"])
    return [b for b in range(first, first + n) if int(src.batches[b]["flags"]) & abi.F_COMPLETE]


def last_offset(b) -> int:
    return _i64(int(b["base_offset"]) + int(b["last_offset_delta"]))


def read_partition(src, segs, rq, entries=None):
    """(status, over_budget, next_offset, returned ordinals) of one partition;
    with FETCH_OFFSETS the last is (expected, actual) of the reference's exception."""
    start, max_offset, max_bytes = int(rq["start_offset"]), int(rq["max_offset"]), int(rq["max_bytes"])
    fl = int(rq["flags"])
    strict = bool(fl & abi.FETCH_STRICT_MAX_BYTES)
    tf = int(rq["type_filter"]) if fl & abi.FETCH_TYPE_FILTER else None
    ft = int(rq["first_timestamp"]) if fl & abi.FETCH_FIRST_TIMESTAMP else None
    consumed, over, got = 0, False, []
    for s in segs:
        chain = chain_of(src, s)
        if not chain:
            continue
        if start > last_offset(src.batches[chain[-1]]):
            continue
        expected = I64_MIN
        at = 0
        if entries is not None:
            pos = find_nearest(entries[s], start)
            if pos is not None:
                at = len(chain)
                for k, b in enumerate(chain):
                    if int(src.batches[b]["file_pos"]) >= pos:
                        at = k
                        break
        for b in chain[at:]:
            h = src.batches[b]
            base, last, size = int(h["base_offset"]), last_offset(h), int(h["size_bytes"])
            if base < expected:
                return abi.FETCH_OFFSETS, over, start, (expected, base)
            if base > max_offset:
                return abi.FETCH_OK, over, start, got
            if (strict or consumed != 0) and ((consumed + size) & M64) > max_bytes:
                return abi.FETCH_OK, True, start, got
            nxt = _i64(last + 1)
            if last < start:
                expected = nxt
                continue
            if (tf is not None and tf != int(h["type"])) or (ft is not None and ft > int(h["first_timestamp"])):
                start = expected = nxt
                continue
            got.append(b)
            start = expected = nxt
            consumed = (consumed + size) & M64
            if last >= max_offset or consumed > max_bytes:
                return abi.FETCH_OK, over, start, got
    return abi.FETCH_OK, over, start, got


@dataclass
class FetchRef:
    out: np.ndarray
    out_part_offsets: np.ndarray
    batches: np.ndarray
    parts: np.ndarray
    totals: np.void
    source: object                                  # the oracle's disk job
    entries: object = None                          # oracle.segment_index's, when the index was used
    returned: list = field(default_factory=list)    # per partition: source ordinals


def expected(oracle, data: np.ndarray, seg_offsets, part_segments, reqs, index_step=None, base_offsets=None,
             flags: int = abi.JOB_CRC, source=None) -> FetchRef:
    """index_step: None reads without the entry index; otherwise the index is
    oracle.segment_index(step=index_step) with base_offsets (default: each
    segment's first batch's base_offset, 0 for a segment without batches)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.asarray(seg_offsets, dtype=np.uint64)
    src = source if source is not None else oracle.run_job(data, offs, flags)
    ps = [int(x) for x in part_segments]
    npart = len(ps) - 1
    reqs = np.asarray(reqs, dtype=abi.FETCH_REQUEST)
    entries = None
    if index_step is not None:
        if base_offsets is None:
            base_offsets = default_base_offsets(src)
        entries = oracle.segment_index(src.batches, src.summaries, base_offsets, step=index_step)
    parts = np.zeros(npart, dtype=abi.FETCH_PART)
    out, out_offs, rows, returned = bytearray(), [0], [], []
    sov = bool(src.totals["overflow"])
    for p in range(npart):
        if sov:
            status, over, nxt, got = abi.FETCH_SOURCE_OVERFLOW, False, int(reqs[p]["start_offset"]), []
        else:
            status, over, nxt, got = read_partition(src, range(ps[p], ps[p + 1]), reqs[p], entries)
        bad = None
        if status == abi.FETCH_OFFSETS:  # the offsets of the reference's exception, nothing returned
            bad, got = got, []
        sel = src.batches[np.asarray(got, dtype=np.int64)] if got else src.batches[:0]
        start = len(out)
        pos = start
        for b, h in zip(got, sel):
            rows.append((pos, b, p))
            pos += int(h["size_bytes"])
        if got:
            out += oracle.serialize_wire(data, offs, sel)
        assert len(out) == pos
        rc = int(np.sum(sel["record_count"].astype(np.int64))) & 0xFFFFFFFF
        parts[p] = (status, int(over), len(got), len(rows) - len(got), rc, len(out) - start,
                    int(sel[0]["base_offset"]) if got else bad[0] if bad else I64_MIN,
                    last_offset(sel[-1]) if got else bad[1] if bad else I64_MIN, nxt,
                    int(sel[0]["first_timestamp"]) if got else -1)
        out_offs.append(len(out))
        returned.append(got)
    tot = np.zeros(1, dtype=abi.FETCH_TOTALS)[0]
    tot["parts_ok"] = int(np.sum(parts["status"] == abi.FETCH_OK))
    tot["batches_out"] = len(rows)
    tot["bytes_out"] = len(out)
    tot["out_capacity_needed"] = len(out) + 16
    tot["out_batch_capacity_needed"] = len(rows)
    return FetchRef(np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.asarray(out_offs, dtype=np.uint64),
                    np.array(rows, dtype=abi.FETCH_BATCH) if rows else np.zeros(0, dtype=abi.FETCH_BATCH), parts, tot,
                    src, entries, returned)


def default_base_offsets(src):
    """A segment's base offset as the log names it: its first batch's."""
    out = []
    for sm in src.summaries:
        first, n = int(sm["first_batch"]), int(sm["n_batches"])
        out.append(int(src.batches[first]["base_offset"]) if n else 0)
    return out


def timequery(oracle, data, seg_offsets, time: int, max_offset: int, source=None):
    """disk_log_impl::timequery (storage/disk_log_impl.cc:861-917) over one
    partition's segments: (offset, time) or None."""
    offs = np.asarray(seg_offsets, dtype=np.uint64)
    src = source if source is not None else oracle.run_job(np.ascontiguousarray(data, dtype=np.uint8), offs, abi.JOB_CRC)
    if offs.size < 2:
        return None
    start = default_base_offsets(src)[0]
    ref = expected(oracle, data, offs, [0, offs.size - 1], requests([request(start, max_offset, 2048, first_timestamp=time)]),
                   source=src)
    p = ref.parts[0]
    if int(p["n_batches"]) and int(p["first_timestamp"]) >= time:
        return int(p["base_offset"]), int(p["first_timestamp"])
    return None
