"""CPU reference of rpgpu_compact: the three reducers of self_compact_segment
restated in plain Python over the oracle's job outputs.

  keep set   compaction_key_reducer with unbounded memory, then
             compacted_offset_list (storage/compaction_reducers.cc:34-114):
             per segment and key, the record last in natural order survives
  filter     copy_data_segment_reducer::filter (:116-222): dropped / verbatim
             / rewritten with model::append_record_to_buffer
             (model/record_utils.cc:183-225) and the rebuilt header
  stamping   reset_size_checksum_metadata through oracle.stamp_batches

tests/test_compaction.py pins this module against the reference's own test
vector and a hand-built batch before the GPU tests compare the device with it.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from redpanda_amd import abi

ELIGIBLE = (abi.F_HEADER_OK | abi.F_COMPLETE | abi.F_CRC_OK | abi.F_PARSED | abi.F_PARSE_OK | abi.F_INDEX_WRITTEN)
M64 = (1 << 64) - 1


def _i64(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


@lru_cache(maxsize=None)
def _vint(v: int) -> bytes:
    from oracle import oracle as O
    return O.vint_serialize(v)


def vint_read(p: bytes, pos: int):
    """vint::deserialize (utils/vint.h:82-98): (value, bytes read); at most
    ten bytes, and at the end of the input whatever was read so far."""
    result = shift = br = 0
    while shift <= 63 and pos + br < len(p):
        byte = p[pos + br]
        br += 1
        if byte & 128:
            result |= ((byte & 127) << shift) & M64
        else:
            result |= (byte << shift) & M64
            break
        shift += 7
    return _i64((result >> 1) ^ (-(result & 1) & M64)), br


def reencode(pay: bytes, rec) -> bytes:
    """model::append_record_to_buffer over the record parse_one_record
    materialises from the bytes at rec_pos: lengths narrowed to int32 as
    model::record stores them, every varint canonical, the bytes of a field
    as far as the payload had them, one empty header for every header the
    count announces past the end of the payload."""
    pos = int(rec["rec_pos"])
    out = bytearray()

    def field(narrow):
        nonlocal pos
        v, br = vint_read(pay, pos)
        pos += br
        st = _i32(v) if narrow else v
        out.extend(_vint(st))
        return v, st

    def blob(v, st):
        nonlocal pos
        if v <= 0 or st <= 0:
            return
        take = min(st, len(pay) - pos)
        out.extend(pay[pos:pos + take])
        pos += take

    field(True)
    if pos < len(pay):
        out.append(pay[pos])
        pos += 1
    field(False)
    field(True)
    blob(*field(True))
    blob(*field(True))
    hcount, _ = field(False)
    for h in range(hcount):
        if pos >= len(pay):
            out.extend(b"\0\0" * (hcount - h))
            break
        blob(*field(True))
        blob(*field(True))
    return bytes(out)


def record_key(pay: bytes, rec) -> bytes:
    kl = int(rec["key_len"])
    if kl <= 0:
        return b""
    kp = int(rec["key_pos"])
    end = min(kp + kl, int(rec["end_pos"]))
    return bytes(pay[kp:min(end, kp + abi.COMPACT_MAX_KEY)])


@dataclass
class RefCompact:
    keep: np.ndarray             # uint64 bitmap over the record-index slots
    out: np.ndarray              # uint8
    out_seg_offsets: np.ndarray  # uint64, n_segments + 1
    batches: np.ndarray          # abi.COMPACT_BATCH
    segments: np.ndarray         # abi.COMPACT_SEGMENT
    totals: np.ndarray           # abi.COMPACT_TOTALS scalar
    kept_offsets: list           # per segment: the surviving record offsets


def payload_of(data, offs, job, b) -> bytes:
    n = int(b["decoded_len"])
    if b["flags"] & abi.F_COMPRESSED:
        o = int(b["decoded_off"])
        return bytes(job.decoded[o:o + n])
    o = int(offs[int(b["segment"])]) + int(b["file_pos"]) + abi.HEADER_SIZE
    return bytes(data[o:o + n])


def segment_status(job, s: int) -> int:
    sm = job.summaries[s]
    fb, nb = int(sm["first_batch"]), int(sm["n_batches"])
    if job.totals["overflow"] or int(sm["first_bad"]) != nb:
        return abi.COMPACT_NOT_CLEAN
    prev = None
    base0 = None
    for b in job.batches[fb:fb + nb]:
        f = int(b["flags"])
        if (f & ELIGIBLE) != ELIGIBLE or (f & abi.F_DECODE_OVERFLOW):
            return abi.COMPACT_NOT_CLEAN
        if (f & abi.F_COMPRESSED) and not (f & abi.F_CODEC_OK):
            return abi.COMPACT_NOT_CLEAN
        if int(b["record_count"]) < 0 or int(b["records_parsed"]) != int(b["record_count"]):
            return abi.COMPACT_NOT_CLEAN
    status = abi.COMPACT_OK
    for b in job.batches[fb:fb + nb]:
        if base0 is None:
            base0 = int(b["base_offset"])
        ib = int(b["index_base"])
        for r in job.records[ib:ib + int(b["record_count"])]:
            o = _i64(int(b["base_offset"]) + int(r["offset_delta"]))
            if not 0 <= ((o - base0) & M64) < (1 << 32):
                status = abi.COMPACT_OFFSETS
            if prev is not None and not o > prev:
                status = abi.COMPACT_OFFSETS
            prev = o
    return status


def compact(data, seg_offsets, job) -> RefCompact:
    """`job`: oracle.run_job(data, seg_offsets, JOB_CRC | JOB_PARSE | JOB_DECODE)
    (or the engine's HostResult of the same job)."""
    from oracle import oracle as O
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.asarray(seg_offsets, dtype=np.uint64)
    nseg = offs.size - 1
    nrec = len(job.records)
    keep = np.zeros((nrec + 63) // 64, dtype=np.uint64)
    out = bytearray()
    seg_off = np.zeros(nseg + 1, dtype=np.uint64)
    entries, positions, plens = [], [], []
    segs = np.zeros(nseg, dtype=abi.COMPACT_SEGMENT)
    kept_offsets = []
    for s in range(nseg):
        seg_off[s] = len(out)
        st = segment_status(job, s)
        segs[s]["status"] = st
        kept_offsets.append([])
        if st != abi.COMPACT_OK:
            continue
        sm = job.summaries[s]
        fb, nb = int(sm["first_batch"]), int(sm["n_batches"])
        bs = job.batches[fb:fb + nb]
        pays = [payload_of(data, offs, job, b) for b in bs]
        # compaction_key_reducer: the last record of every key, in natural order
        last = {}
        for b, pay in zip(bs, pays):
            ib = int(b["index_base"])
            for slot in range(ib, ib + int(b["record_count"])):
                last[record_key(pay, job.records[slot])] = slot
        kept = set(last.values())
        for slot in kept:
            keep[slot >> 6] |= np.uint64(1 << (slot & 63))
        start = len(out)
        n_out = n_rw = 0
        for k, (b, pay) in enumerate(zip(bs, pays)):
            ib, rc = int(b["index_base"]), int(b["record_count"])
            mine = [slot for slot in range(ib, ib + rc) if slot in kept]
            kept_offsets[s] += [_i64(int(b["base_offset"]) + int(job.records[x]["offset_delta"])) for x in mine]
            if not mine:
                continue
            first_ts, max_ts = int(b["first_timestamp"]), int(b["max_timestamp"])
            attrs = int(b["attrs"]) & 0xFFFF
            if len(mine) == rc:
                body = pay
            else:
                body = b"".join(reencode(pay, job.records[x]) for x in mine)
                first_ts = _i64(first_ts + int(job.records[mine[0]]["ts_delta"]))
                if not attrs & 8:
                    max_ts = _i64(first_ts + int(job.records[mine[-1]]["ts_delta"]))
                n_rw += 1
            hdr = struct.pack("<IiqbiHiqqqhii", 0, 0, int(b["base_offset"]), int(b["type"]), 0, attrs & ~7 & 0xFFFF,
                              int(b["last_offset_delta"]), first_ts, max_ts, int(b["producer_id"]),
                              int(b["producer_epoch"]), int(b["base_sequence"]), len(mine))
            assert len(hdr) == abi.HEADER_SIZE
            e = np.zeros(1, dtype=abi.COMPACT_BATCH)[0]
            e["out_pos"], e["src_batch"], e["payload_len"] = len(out), fb + k, len(body)
            e["codec"], e["kept"] = attrs & 7, len(mine)
            e["flags"] = abi.COMPACT_F_REWRITTEN if len(mine) != rc else 0
            entries.append(e)
            positions.append(len(out))
            plens.append(len(body))
            out += hdr + body
            n_out += 1
        g = segs[s]
        g["records_in"] = sum(int(b["record_count"]) for b in bs)
        g["records_kept"] = len(kept)
        g["batches_in"], g["batches_out"], g["batches_rewritten"] = nb, n_out, n_rw
        g["bytes_out"] = len(out) - start
    seg_off[nseg] = len(out)
    buf = np.frombuffer(bytes(out) + b"\0" * 16, dtype=np.uint8)
    if positions:
        buf = O.stamp_batches(buf, positions, plens, 0, abi.STAMP_CRC)
    tot = np.zeros(1, dtype=abi.COMPACT_TOTALS)[0]
    for f in ("records_in", "records_kept", "batches_in", "batches_out", "batches_rewritten", "bytes_out"):
        tot[f] = int(np.sum(segs[f].astype(np.uint64)))
    tot["out_capacity_needed"] = len(out) + 16
    tot["out_batch_capacity_needed"] = len(entries)
    bat = np.array(entries, dtype=abi.COMPACT_BATCH) if entries else np.zeros(0, dtype=abi.COMPACT_BATCH)
    return RefCompact(keep, np.array(buf[:len(out)]), seg_off, bat, segs, tot, kept_offsets)
