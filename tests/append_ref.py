"""CPU reference of rpgpu_append_wire, from pieces that already exist:

  verdicts   the rules of include/rpgpu.h (rpgpu_append_status) over the
             oracle's wire-layout job (kafka::batch_reader +
             kafka_batch_adapter::adapt, kafka/protocol/kafka_batch_adapter.cc:
             32-188; the partition verdict of produce.cc:364-412)
  headers    the adapted disk header (storage/segment_appender_utils.cc:28-54)
             in front of the wire payload; set_max_timestamp (model/record.h:
             598-608) for sets with an append time
  stamping   disk_log_appender::operator() through oracle.stamp_batches
             (offsets; offsets + crc where set_max_timestamp ran; header_crc)
  metadata   the oracle's disk-layout job over the result

tests/test_append.py checks this module against itself and the reference's
record_batch_test.cc vector before the GPU tests compare the device with it.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from redpanda_amd import abi
from tests import batchgen as bg

M64 = (1 << 64) - 1
TS0 = 1600000000000


def _i64(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _crc():
    from oracle import oracle as O
    O.build()
    return O.crc32c


def wire_batch(payload: bytes, record_count: int, *, attrs: int = 0, base_offset: int = 0, lod: int | None = None,
               first_ts: int = TS0, max_ts: int | None = None, pid: int = -1, epoch: int = -1, seq: int = -1,
               magic: int = 2, crc: int | None = None, batch_length: int | None = None) -> bytes:
    """One Kafka v2 wire batch (kafka/protocol/response_writer.h:241-276);
    crc and batch_length are computed unless given."""
    lod = record_count - 1 if lod is None else lod
    max_ts = first_ts + max(record_count - 1, 0) if max_ts is None else max_ts
    prefix = bg.be_prefix(attrs, lod, first_ts, max_ts, pid, epoch, seq, record_count)
    if crc is None:
        c = _crc()
        crc = c(payload, c(prefix))
    blen = 49 + len(payload) if batch_length is None else batch_length
    return struct.pack(">qiibI", base_offset, blen, 0, magic, crc & 0xFFFFFFFF) + prefix + bytes(payload)


def batch_verdict(flags: int) -> int:
    """rpgpu_append_status of one batch of a wire-layout job."""
    if not flags & abi.F_COMPLETE:
        return abi.APPEND_MALFORMED
    if not flags & abi.F_WIRE_V2:
        return abi.APPEND_CORRUPT_MESSAGE
    if not flags & abi.F_CRC_OK:
        return abi.APPEND_CORRUPT_MESSAGE
    if flags & abi.F_CODEC_INVALID:
        return abi.APPEND_MALFORMED
    if not flags & abi.F_COMPRESSED and not flags & abi.F_PARSE_OK:
        return abi.APPEND_INVALID_RECORD
    return abi.APPEND_OK


def set_verdict(batches, summary, all_batches: bool):
    """(status, first_bad, chain ordinals appended) of one record set."""
    n = len(batches)
    v = [batch_verdict(int(b["flags"])) for b in batches]
    if not all_batches:
        if n == 0:
            return abi.APPEND_MALFORMED, 0, []
        if v[0] != abi.APPEND_OK:
            return v[0], 0, []
        return abi.APPEND_OK, n, [0]
    for i, x in enumerate(v):
        if x != abi.APPEND_OK:
            return x, i, []
    if int(summary["terminal_errc"]) != abi.ERRC_END_OF_STREAM:
        return abi.APPEND_MALFORMED, n, []
    return abi.APPEND_OK, n, list(range(n))


@dataclass
class AppendRef:
    out: np.ndarray
    out_seg_offsets: np.ndarray
    batches: np.ndarray
    summaries: np.ndarray
    sets: np.ndarray
    totals: np.void
    source: object                      # the oracle's wire job
    accepted: list = field(default_factory=list)   # (set, wire offset in data, size_bytes) per appended batch


def expected(oracle, data: np.ndarray, seg_offsets, next_offsets, append_times=None, all_batches: bool = False,
             flags: int = abi.JOB_CRC | abi.JOB_PARSE) -> AppendRef:
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.asarray(seg_offsets, dtype=np.uint64)
    nseg = offs.size - 1
    src = oracle.run_job(data, offs, flags, layout=abi.LAYOUT_WIRE)
    assert not src.totals["overflow"]
    raw = data.tobytes()
    sets = np.zeros(nseg, dtype=abi.APPEND_SET)
    out = bytearray()
    out_offs = [0]
    accepted, src_ord = [], []
    stamps = []  # per set: (positions, payload lens, next offset, flags)
    for s in range(nseg):
        sm = src.summaries[s]
        first, n = int(sm["first_batch"]), int(sm["n_batches"])
        chain = src.batches[first:first + n]
        status, first_bad, take = set_verdict(chain, sm, all_batches)
        t = None
        if append_times is not None and int(append_times[s]) != abi.APPEND_CREATE_TIME:
            t = int(append_times[s])
        pos, plen, steps = [], [], 0
        start = len(out)
        for k in take:
            b = chain[k]
            w = int(offs[s]) + int(b["file_pos"])
            size = int(b["size_bytes"])
            (base, blen, ple, magic, crc, attrs, lod, fts, mts, pid, epoch, seq, rc) = bg.WIRE_HDR.unpack_from(raw, w)
            assert blen + 12 == size
            if t is not None:  # set_max_timestamp(append_time, t)
                attrs = struct.unpack("<h", struct.pack("<H", (attrs & 0xFFFF) | 8))[0]
                mts = t
            pos.append(len(out))
            plen.append(size - 61)
            out += bg.DISK_HDR.pack(0, size, 0, 1, crc, attrs, lod, fts, mts, pid, epoch, seq, rc)
            out += raw[w + 61:w + size]
            steps += lod + 1
            accepted.append((s, w, size))
            src_ord.append(first + k)
        nxt = int(next_offsets[s])
        if pos:
            stamps.append((pos, plen, nxt, abi.STAMP_OFFSETS | (abi.STAMP_CRC if t is not None else 0)))
        sets[s] = (status, first_bad, len(take), nxt, _i64(nxt + steps - 1), len(out) - start)
        out_offs.append(len(out))
    buf = np.frombuffer(bytes(out), dtype=np.uint8).copy()
    for pos, plen, nxt, fl in stamps:  # each set's own bytes: its appender starts at its next_offset
        a, e = pos[0], pos[-1] + 61 + plen[-1]
        buf[a:e] = oracle.stamp_batches(buf[a:e], [p - a for p in pos], plen, nxt, fl)
    out_offs = np.asarray(out_offs, dtype=np.uint64)
    disk = oracle.run_job(buf, out_offs, flags)
    assert len(disk.batches) == len(accepted)
    eb = disk.batches.copy()
    so = np.asarray(src_ord, dtype=np.int64)
    if len(eb):
        eb["index_base"] = src.batches["index_base"][so]
        eb["decoded_off"] = src.batches["decoded_off"][so]
        eb["decoded_crc"] = 0
        eb["decoded_header_crc"] = 0
    es = disk.summaries.copy()
    es["n_records"] = 0
    tot = np.zeros(1, dtype=abi.APPEND_TOTALS)[0]
    tot["sets_ok"] = int(np.sum(sets["status"] == abi.APPEND_OK))
    tot["batches_out"] = len(accepted)
    tot["bytes_out"] = buf.size
    tot["out_capacity_needed"] = buf.size + 16
    tot["out_batch_capacity_needed"] = len(accepted)
    return AppendRef(buf, out_offs, eb, es, sets, tot, src, accepted)


def set_max_timestamp(oracle, batch: bytes, append_time: bool, ts: int) -> bytes:
    """record_batch::set_max_timestamp (model/record.h:598-608) over one
    disk-layout batch: attrs bit 3 and max_timestamp, then crc_record_batch and
    internal_header_only_crc through oracle.stamp_batches."""
    b = bytearray(batch)
    attrs = struct.unpack_from("<H", b, 21)[0]
    struct.pack_into("<H", b, 21, (attrs | 8) if append_time else (attrs & ~8 & 0xFFFF))
    struct.pack_into("<q", b, 35, ts)
    arr = np.frombuffer(bytes(b), dtype=np.uint8)
    return oracle.stamp_batches(arr, [0], [len(b) - 61], 0, abi.STAMP_CRC).tobytes()
