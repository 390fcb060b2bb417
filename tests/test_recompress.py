"""Recompression of compacted batches (rpgpu_recompress).

CPU tests check the ABI and pin the Python model (tests/recompress_ref.py)
against liblz4 (through oracle/_ref) and against the oracle's own decoder.
GPU tests compare the device with that model byte for byte and field for
field: output bytes, segment offsets, entries, batch results, summaries and
totals; then run the device's output back through the validator and the
segment index.

The payload sizes at the edges of the block code (1, 12, 13 bytes ...) cannot
be the payload of a batch that parses, so compaction never returns them: those
tests lay the batches out as rpgpu_compact's outputs by hand (a stamped header
in front of the bytes, an entry per batch) and start at rpgpu_recompress.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from redpanda_amd import abi
from tests import batchgen as BG
from tests import compaction_ref as CR
from tests import compress_edges as CE
from tests import recompress_ref as RR
from tests import test_compaction as TC

DFLAGS = abi.JOB_CRC | abi.JOB_PARSE | abi.JOB_DECODE
GOOD = abi.F_HEADER_OK | abi.F_COMPLETE | abi.F_CRC_OK
EDGE_SIZES = [1, 12, 13, 64, 65535, 65536, 65537, 2 * 65536 + 1]


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def laid_out(payloads, codecs, seg_counts=None):
    """A RefCompact holding one uncompressed batch per payload (header stamped
    by batchgen), entry codec codecs[i]; seg_counts: batches per segment."""
    from oracle import oracle as O
    out = bytearray()
    ents = np.zeros(len(payloads), dtype=abi.COMPACT_BATCH)
    for i, (p, c) in enumerate(zip(payloads, codecs)):
        ents[i]["out_pos"], ents[i]["src_batch"], ents[i]["payload_len"] = len(out), i, len(p)
        ents[i]["codec"], ents[i]["kept"] = c, 1
        crc = O.crc32c(bytes(p), O.crc32c(BG.be_prefix(0, 0, TC.TS0 + i, TC.TS0 + i, -1, -1, -1, 1)))
        out += BG.batch(bytes(p), 1, base_offset=10 * i, first_ts=TC.TS0 + i, crc=crc)
    seg_counts = [len(payloads)] if seg_counts is None else seg_counts
    offs, k = [0], 0
    for n in seg_counts:
        k += n
        offs.append(int(ents[k]["out_pos"]) if k < len(ents) else len(out))
    tot = np.zeros(1, dtype=abi.COMPACT_TOTALS)[0]
    tot["batches_out"] = tot["out_batch_capacity_needed"] = len(ents)
    tot["bytes_out"] = len(out)
    tot["out_capacity_needed"] = len(out) + 16
    return CR.RefCompact(np.zeros(0, np.uint64), np.frombuffer(bytes(out), dtype=np.uint8).copy(),
                         np.array(offs, dtype=np.uint64), ents, np.zeros(len(seg_counts), dtype=abi.COMPACT_SEGMENT),
                         tot, [])


def to_device(cref, spare_batches=2):
    """The engine's CompactResult of a RefCompact."""
    import torch
    from redpanda_amd.engine import CompactResult
    cap = cref.out.size + 16
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out[: cref.out.size] = torch.from_numpy(cref.out)
    ents = np.zeros(len(cref.batches) + spare_batches, dtype=abi.COMPACT_BATCH)
    ents[: len(cref.batches)] = cref.batches
    nseg = len(cref.out_seg_offsets) - 1
    return CompactResult(
        keep=None, out=out, out_seg_offsets=torch.from_numpy(cref.out_seg_offsets.view(np.int64).copy()).cuda(),
        batches=torch.from_numpy(ents.view(np.uint8).copy()).cuda(), segments=None,
        totals=torch.from_numpy(np.array([cref.totals]).view(np.uint8).copy()).cuda(), n_segments=nseg, n_records=0,
        out_capacity=cap)


def edge_payloads():
    rng = np.random.default_rng(0xEDCE)
    return [np.zeros(n, np.uint8).tobytes() for n in EDGE_SIZES] + \
           [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in EDGE_SIZES]


def coded_batch(O, records, base, codec, payload):
    """A disk batch whose stored payload is `payload` (the records compressed by the caller)."""
    n = len(records)
    crc = O.crc32c(payload, O.crc32c(BG.be_prefix(codec, n - 1, TC.TS0, TC.TS0 + max(n - 1, 0), -1, -1, -1, n)))
    return BG.batch(payload, n, base_offset=base, attrs=codec, first_ts=TC.TS0, crc=crc)


def gzip_bytes(raw):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(raw) + c.flush()


def host_codec_segment(O):
    """gzip and zstd sources beside an uncompressed one: per codec a partly
    kept and a fully kept batch.  zstd only where libzstd is there to make
    the frames."""
    coders = [(abi.CODEC_GZIP, gzip_bytes)]
    try:
        from tests import zstd_corpus as ZC
        ZC.frame(b"probe")
        coders.append((abi.CODEC_ZSTD, ZC.frame))
    except OSError:
        pass
    batches, off = [], 0
    for i, (codec, enc) in enumerate(coders):
        for keys in ([b"k%d" % i, b"dup"], [b"whole%d" % i, b"other%d" % i]):
            recs = [BG.record(j, k, bytes([65 + i]) * 300) for j, k in enumerate(keys)]
            batches.append(coded_batch(O, recs, off, codec, enc(b"".join(recs))))
            off += len(recs)
    batches.append(TC.keyed_batch(O, [b"dup", b"plain"], off, vlen=200, seed=9))
    return TC.as_seg(batches), [c for c, _ in coders]


def assert_model_parity(got, ref):
    np.testing.assert_array_equal(got.out_seg_offsets, ref.out_seg_offsets, err_msg="out_seg_offsets")
    for f in abi.RECOMPRESS_TOTALS_COMPARE_FIELDS:
        assert int(got.totals[f]) == int(ref.totals[f]), f"totals.{f}"
    assert len(got.entries) == len(ref.entries)
    for f in abi.RECOMPRESS_BATCH_COMPARE_FIELDS:
        np.testing.assert_array_equal(got.entries[f], ref.entries[f], err_msg=f"entries.{f}")
    assert got.out.size == ref.out.size
    bad = np.nonzero(got.out != ref.out)[0]
    assert bad.size == 0, f"output bytes differ first at {bad[:8]}"
    # what a JOB_CRC job over the output reports: memcmp-equal, reserved fields included
    assert got.batches.tobytes() == ref.batches.tobytes(), [
        f for f in abi.BATCH_RESULT.names if not np.array_equal(got.batches[f], ref.batches[f])]
    assert got.summaries.tobytes() == ref.summaries.tobytes(), [
        f for f in abi.SEGMENT_SUMMARY.names if not np.array_equal(got.summaries[f], ref.summaries[f])]


def model_payloads(ref):
    return [ref.out[int(e["out_pos"]) + 61:int(e["out_pos"]) + 61 + int(e["payload_len"])].tobytes() for e in ref.entries]


def compact_payloads(cref):
    return [cref.out[int(e["out_pos"]) + 61:int(e["out_pos"]) + 61 + int(e["payload_len"])].tobytes() for e in cref.batches]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_abi_exports_and_sizes(rplib):
    L = rplib.load()
    for name in ("rpgpu_recompress", "rpgpu_recompress_sizeof", "rpgpu_recompress_timings"):
        assert hasattr(L, name), name
        assert name in rplib.exported_symbols_from_header()
    assert [L.rpgpu_recompress_sizeof(i) for i in range(5)] == [
        abi.RECOMPRESS_BATCH.itemsize, abi.RECOMPRESS_TOTALS.itemsize, abi.BATCH_RESULT.itemsize,
        C.sizeof(rplib.RecompressJobC), 0]
    assert L.rpgpu_recompress(None, None, None) == abi.E_INVALID
    job = rplib.RecompressJobC()
    job.snappy_frag = 100
    assert L.rpgpu_recompress(None, C.byref(job), None) == abi.E_INVALID
    assert L.rpgpu_recompress_timings(None, None, 0) == abi.E_INVALID


def lz4_source_refs(O):
    """test_compaction's reference vector and its hand-built partly kept batch, from LZ4 source batches."""
    k1, k2 = b"\x01" * 1024, b"\x02" * 1024
    vec = [TC.keyed_batch(O, [k1 if (b * 10 + i) % 2 == 0 else k2 for i in range(10)], b * 10, codec=abi.CODEC_LZ4,
                          seed=b) for b in range(10)]
    recs = [BG.record(i, k, v) for i, (k, v) in enumerate(zip([b"a", b"b", b"a", b"c"], [b"v0", b"v1", b"v2", b"v3"]))]
    hand = [TC.make_batch(O, recs, 7, codec=abi.CODEC_LZ4)]
    out = []
    for bs in (vec, hand):
        seg = TC.as_seg(bs)
        offs = np.array([0, seg.size], dtype=np.uint64)
        # the decode arena reserves a whole 64 KiB block per LZ4 block
        job = O.run_job(seg, offs, DFLAGS, decoded_cap=len(bs) << 16)
        out.append(CR.compact(seg, offs, job))
        assert out[-1].segments[0]["status"] == abi.COMPACT_OK
    return out


def test_model_matches_the_libraries(oracle):
    O = oracle
    for cref in lz4_source_refs(O):
        assert len(cref.batches) >= 1 and all(int(c) == abi.CODEC_LZ4 for c in cref.batches["codec"])
        ref = RR.recompress(cref)
        assert all(int(f) == abi.RECOMPRESS_F_COMPRESSED for f in ref.entries["flags"])
        assert int(ref.totals["batches_compressed"]) == len(cref.batches)
        want = compact_payloads(cref)
        if O.ref() is not None:  # liblz4 itself
            for got, raw in zip(model_payloads(ref), want):
                assert got == O.ref_compress(abi.CODEC_LZ4, raw)
        # the output is a log the reference's reader accepts and decodes to the compacted payloads
        job = O.run_job(ref.out, ref.out_seg_offsets, DFLAGS)
        assert len(job.batches) == len(want)
        full = GOOD | abi.F_COMPRESSED | abi.F_CODEC_OK | abi.F_PARSE_OK
        assert np.all((job.batches["flags"] & full) == full)
        for b, raw in zip(job.batches, want):
            o, n = int(b["decoded_off"]), int(b["decoded_len"])
            assert job.decoded[o:o + n].tobytes() == raw
        # every header field but attrs' codec, size and the crcs is the compacted batch's
        for e, c in zip(ref.entries, cref.batches):
            h0 = BG.HDR.unpack(cref.out[int(c["out_pos"]):int(c["out_pos"]) + 61].tobytes())
            h1 = BG.HDR.unpack(ref.out[int(e["out_pos"]):int(e["out_pos"]) + 61].tobytes())
            assert h1[5] == h0[5] | abi.CODEC_LZ4 and h1[1] == 61 + int(e["payload_len"])
            assert h1[2:4] == h0[2:4] and h1[6:] == h0[6:]


def test_threshold_and_override(oracle):
    O = oracle
    pays = [bytes(139), bytes(138), bytes(140)]
    cref = laid_out(pays, [abi.CODEC_LZ4] * 3)
    ref = RR.recompress(cref, min_batch_bytes=200)  # 61 + 139 = 200: at the threshold
    assert [int(f) for f in ref.entries["flags"]] == [abi.RECOMPRESS_F_COMPRESSED, 0, abi.RECOMPRESS_F_COMPRESSED]
    assert [int(c) for c in ref.entries["codec"]] == [abi.CODEC_LZ4, abi.CODEC_NONE, abi.CODEC_LZ4]
    p = int(ref.entries[1]["out_pos"])
    q = int(cref.batches[1]["out_pos"])
    assert ref.out[p:p + 61 + 138].tobytes() == cref.out[q:q + 61 + 138].tobytes()
    assert model_payloads(ref)[0] == O.compress(abi.CODEC_LZ4, pays[0])
    none = RR.recompress(cref, codec=abi.CODEC_NONE)
    assert none.out.tobytes() == cref.out.tobytes() and not np.any(none.entries["flags"])
    assert int(none.totals["batches_compressed"]) == 0
    host = RR.recompress(cref, codec=abi.CODEC_ZSTD)
    assert host.out.tobytes() == cref.out.tobytes() and int(host.totals["batches_host"]) == 3
    assert np.all(host.batches["flags"] == GOOD)  # still uncompressed: a valid log


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def run_device(engine, dcomp, **kw):
    import torch
    dev = engine.recompress(dcomp, **kw)
    torch.cuda.synchronize()
    return dev.to_host(), dev


def assert_closure(engine, O, got, ref, want_payloads, parse):
    """The device's output validates, decodes to the compacted payloads and indexes as the model's job does."""
    import torch
    if got.out.size:
        d = torch.from_numpy(np.concatenate([got.out, np.zeros(16, np.uint8)])).cuda()[: got.out.size]
        flags = abi.JOB_CRC | abi.JOB_DECODE | (abi.JOB_PARSE if parse else 0)
        v = engine.validate(d, got.out_seg_offsets, flags)
        assert len(v.batches) == len(want_payloads)
        for b, raw in zip(v.batches, want_payloads):
            f, n = int(b["flags"]), int(b["decoded_len"])
            assert (f & GOOD) == GOOD and not f & (abi.F_CODEC_INVALID | abi.F_DECODE_OVERFLOW)
            assert not parse or f & abi.F_PARSE_OK
            if f & abi.F_COMPRESSED:
                assert f & abi.F_CODEC_OK
                o = int(b["decoded_off"])
                assert v.decoded[o:o + n].tobytes() == raw
            else:
                o = int(got.out_seg_offsets[int(b["segment"])]) + int(b["file_pos"]) + 61
                assert n == len(raw) and got.out[o:o + n].tobytes() == raw


def assert_index(engine, O, dev, ref, steps=(1, abi.INDEX_DEFAULT_STEP)):
    nseg = dev.n_segments
    bases = [int(ref.batches[int(s["first_batch"])]["base_offset"]) if int(s["n_batches"]) else 0 for s in ref.summaries]
    cap = dev.batches.numel() // abi.BATCH_RESULT.itemsize
    for step in steps:
        gix = engine.index_to_host(*engine.segment_index(dev, bases, step=step), n_segments=nseg)
        rix = O.segment_index(ref.batches, ref.summaries, bases, step=step, batch_cap=cap)
        for (gs, gro, grt, gps), (rs, rro, rrt, rps) in zip(gix, rix):
            assert all(int(gs[f]) == int(rs[f]) for f in abi.INDEX_STATE.names), ("index state", step)
            assert np.array_equal(gro, rro) and np.array_equal(grt, rrt) and np.array_equal(gps, rps), step


@pytest.mark.gpu
@pytest.mark.parametrize("codec,frag", [(abi.CODEC_LZ4, 0), (abi.CODEC_SNAPPY, 0), (abi.CODEC_SNAPPY, 4096),
                                        (abi.CODEC_SNAPPY, 65537)])
def test_gpu_edge_sizes(engine, oracle, codec, frag):
    """Payloads of 1, 12, 13 (LZ4's all-literal limit), 64, 65535, 65536, 65537
    and 2 * 65536 + 1 bytes, all-zero and random (LZ4's raw-block branch, the
    compressed form larger than the input), two segments; the codec comes
    through the override."""
    pays = edge_payloads()
    cref = laid_out(pays, [abi.CODEC_NONE] * len(pays), seg_counts=[len(EDGE_SIZES), len(EDGE_SIZES)])
    ref = RR.recompress(cref, codec=codec, snappy_frag=frag)
    got, dev = run_device(engine, to_device(cref), codec=codec, snappy_frag=frag)
    assert int(got.totals["overflow"]) == 0
    assert_model_parity(got, ref)
    assert np.all(got.entries["flags"] == abi.RECOMPRESS_F_COMPRESSED)
    grew = got.entries["payload_len"] > got.entries["in_payload_len"]
    assert grew[len(EDGE_SIZES):].all(), "random bytes: the compressed form is larger and is kept"
    assert_closure(engine, oracle, got, ref, pays, parse=False)
    assert_index(engine, oracle, dev, ref)


# One case per LZ4 output-limit exit and the exact-fit pair (raw blocks are
# copied from where the payload lies in the log, unstaged), and the cases whose
# match ends at lane 63 / 0 of wave_count's second and third step, by a
# mismatch and by the end of the block, for both codecs.
ALIGN_CASES = ["lz4_exit1_literal_run", "lz4_exit2_match_length", "lz4_exit3_last_literals", "lz4_raw_at_n",
               "lz4_fits_n_minus_1", "lz4_match_67", "lz4_match_68", "lz4_match_132", "lz4_mlimit_run_137",
               "lz4_mlimit_run_138", "snappy_copy_67", "snappy_copy_68", "snappy_copy_132", "snappy_end_run_132",
               "snappy_end_run_133"]
_aligned = {}


def aligned_layout():
    """Every ALIGN_CASES payload 16 times, each behind a filler batch of 0..15
    payload bytes chosen so that the payload starts at residue r = 0..15 mod 16
    of the log: (cref, payloads, [(case, r, batch ordinal)])."""
    if not _aligned:
        edge = dict(CE.cases())
        rng = np.random.default_rng(0xA119)
        pays, where, pos = [], [], 0
        for name in ALIGN_CASES:
            for r in range(16):
                f = (r - (pos + 2 * abi.HEADER_SIZE)) % 16
                pays += [rng.integers(0, 256, f, dtype=np.uint8).tobytes(), edge[name]]
                where.append((name, r, len(pays) - 1))
                pos += 2 * abi.HEADER_SIZE + f + len(edge[name])
        third = len(pays) // 3 // 2 * 2
        cref = laid_out(pays, [abi.CODEC_NONE] * len(pays), seg_counts=[third, third, len(pays) - 2 * third])
        _aligned.update(cref=cref, pays=pays, where=where)
    return _aligned["cref"], _aligned["pays"], _aligned["where"]


@pytest.mark.gpu
@pytest.mark.parametrize("codec,frag", [(abi.CODEC_LZ4, 0), (abi.CODEC_SNAPPY, 0), (abi.CODEC_SNAPPY, 4097)])
def test_gpu_payload_alignments(engine, oracle, codec, frag):
    """The block compressors read a payload where it lies in the log (g32 from
    the absolute address) and raw LZ4 blocks are copied from there: every
    residue mod 16 of the payload's first byte in the device buffer, for the
    edge payloads of ALIGN_CASES."""
    cref, pays, where = aligned_layout()
    dcomp = to_device(cref)
    base = dcomp.out.data_ptr()
    assert base % 16 == 0
    seen = {}
    for name, r, b in where:
        start = base + int(cref.batches[b]["out_pos"]) + abi.HEADER_SIZE
        assert start % 16 == r and int(cref.batches[b - 1]["payload_len"]) < 16
        seen.setdefault(name, set()).add(start % 16)
    assert seen == {name: set(range(16)) for name in ALIGN_CASES}
    ref = RR.recompress(cref, codec=codec, snappy_frag=frag)
    got, dev = run_device(engine, dcomp, codec=codec, snappy_frag=frag)
    assert int(got.totals["overflow"]) == 0
    assert_model_parity(got, ref)
    assert np.all(got.entries["flags"] == abi.RECOMPRESS_F_COMPRESSED)
    if codec == abi.CODEC_LZ4:  # the exits' blocks are stored raw: the frame is the payload and 23 bytes
        for name, r, b in where:
            if name.startswith("lz4_exit") or name == "lz4_raw_at_n":
                assert int(got.entries[b]["payload_len"]) == len(pays[b]) + 23, (name, r)
    assert_closure(engine, oracle, got, ref, pays, parse=False)
    assert_index(engine, oracle, dev, ref)


def scale_layout(cu):
    """cu * 32 + 307 batches of at most 32 payload bytes (none / LZ4 / snappy
    by turns, one gzip), three uncompressed ones of 65535, 65536 and
    3 * 65536 + 5 bytes, over 300 segments of which every ninth is empty."""
    n_tiny = cu * 32 + 307
    rng = np.random.default_rng(0x5CA1E)
    pays, codecs = [], []
    for i in range(n_tiny):
        n = int(rng.integers(0, 33))
        pays.append(bytes([i & 255]) * n if i % 5 == 0 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        codecs.append((abi.CODEC_NONE, abi.CODEC_LZ4, abi.CODEC_SNAPPY)[i % 3])
    codecs[1000] = abi.CODEC_GZIP
    big = {97: 65535, n_tiny // 2: 65536, n_tiny - 40: 3 * 65536 + 5}
    for at, size in sorted(big.items()):
        pays.insert(at, rng.integers(0, 256, size - abi.HEADER_SIZE, dtype=np.uint8).tobytes())
        codecs.insert(at, abi.CODEC_NONE)
    nb, nseg = len(pays), 300
    full = [s for s in range(nseg) if s % 9 != 4]
    seg_counts = [0] * nseg
    for s in full:
        seg_counts[s] = nb // len(full)
    seg_counts[full[-1]] += nb - sum(seg_counts)
    assert sum(seg_counts) == nb and seg_counts.count(0) > 30 and nseg > 256
    return laid_out(pays, codecs, seg_counts=seg_counts), pays, codecs


@pytest.mark.gpu
def test_gpu_scale(engine, oracle):
    """One call past every single-block limit of the recompress kernels: more
    batches than one 256-thread block of the thread-per-batch kernels, more
    than 256 segments (some empty) for k_recompress_layout, more pack pieces
    than k_recompress_pack's grid has waves (cu_count * 32: its grid-stride
    loop), and copied batches of 65535, 65536 (one piece) and 3 * 65536 + 5
    bytes (four pieces).  The codecs come from the entries."""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    cref, pays, codecs = scale_layout(cu)
    nb = len(pays)
    ref = RR.recompress(cref)
    pieces = sum(1 if int(e["flags"]) & abi.RECOMPRESS_F_COMPRESSED else -(-(abi.HEADER_SIZE + int(e["payload_len"])) // 65536)
                 for e in ref.entries)
    assert pieces > cu * 32 and pieces == nb + 3
    got, dev = run_device(engine, to_device(cref))
    assert int(got.totals["overflow"]) == 0
    assert_model_parity(got, ref)
    assert int(got.totals["batches_host"]) == 1
    assert int(got.totals["batches_compressed"]) == sum(1 for c in codecs if c in (abi.CODEC_LZ4, abi.CODEC_SNAPPY))
    copied = 0
    for e in got.entries:
        if not int(e["flags"]) & abi.RECOMPRESS_F_COMPRESSED:
            s = cref.batches[int(e["in_batch"])]
            n = abi.HEADER_SIZE + int(s["payload_len"])
            assert got.out[int(e["out_pos"]):int(e["out_pos"]) + n].tobytes() == \
                cref.out[int(s["out_pos"]):int(s["out_pos"]) + n].tobytes(), int(e["in_batch"])
            copied += 1
    assert copied == sum(1 for c in codecs if c in (abi.CODEC_NONE, abi.CODEC_GZIP))
    assert_index(engine, oracle, dev, ref, steps=(1,))


_chain = {}


def real_chain(engine, O):
    """test_compaction's mixed segments (none / LZ4 + snappy sources, one
    segment not clean), an empty segment and the gzip / zstd sources, through
    submit -> compact -> recompress(SOURCE_CODEC); run once."""
    if not _chain:
        seg, host_codecs = host_codec_segment(O)
        mixed = TC.mixed_segments(O)
        segs = mixed[:2] + [np.zeros(0, np.uint8)] + mixed[2:] + [seg]
        chost, cref, job, dcomp = TC.run_device(engine, O, segs)
        TC.assert_parity(chost, cref)
        ref = RR.recompress(cref)
        got, dev = run_device(engine, dcomp)
        _chain.update(cref=cref, ref=ref, got=got, dev=dev, dcomp=dcomp, host_codecs=host_codecs)
    return _chain


@pytest.mark.gpu
def test_gpu_real_chain(engine, oracle):
    c = real_chain(engine, oracle)
    cref, ref, got = c["cref"], c["ref"], c["got"]
    assert [int(s) for s in cref.segments["status"]] == [0, 0, 0, abi.COMPACT_NOT_CLEAN, 0]
    assert_model_parity(got, ref)
    flags = {int(k): [int(f) for f in got.entries["flags"][got.entries["codec"] == k]] for k in range(5)}
    assert flags[abi.CODEC_NONE] and not any(flags[abi.CODEC_NONE])
    for k in (abi.CODEC_LZ4, abi.CODEC_SNAPPY):
        assert len(flags[k]) >= 2 and set(flags[k]) == {abi.RECOMPRESS_F_COMPRESSED}
    n_host = 0
    for k in c["host_codecs"]:
        assert len(flags[k]) == 2 and set(flags[k]) == {abi.RECOMPRESS_F_HOST}
        n_host += 2
    assert int(got.totals["batches_host"]) == n_host >= 2
    # the host's batches (and the uncompressed ones): verbatim
    for e in got.entries:
        if not int(e["flags"]) & abi.RECOMPRESS_F_COMPRESSED:
            s = cref.batches[int(e["in_batch"])]
            n = 61 + int(s["payload_len"])
            assert got.out[int(e["out_pos"]):int(e["out_pos"]) + n].tobytes() == \
                cref.out[int(s["out_pos"]):int(s["out_pos"]) + n].tobytes()
    # the empty and the unclean segment are empty, with an empty segment's summary
    for s in (2, 3):
        assert int(got.out_seg_offsets[s]) == int(got.out_seg_offsets[s + 1])
        assert int(got.summaries[s]["n_batches"]) == 0 and int(got.summaries[s]["has_checkpoint"]) == 0


@pytest.mark.gpu
def test_gpu_closure(engine, oracle):
    c = real_chain(engine, oracle)
    assert_closure(engine, oracle, c["got"], c["ref"], compact_payloads(c["cref"]), parse=True)
    assert_index(engine, oracle, c["dev"], c["ref"])


@pytest.mark.gpu
def test_gpu_capacities(engine, oracle):
    import torch
    pays = [bytes(range(256)) * 3, bytes(5000), b"xyz" * 100]
    cref = laid_out(pays, [abi.CODEC_LZ4, abi.CODEC_SNAPPY, abi.CODEC_NONE])
    ref = RR.recompress(cref)
    need, nbat = int(ref.totals["out_capacity_needed"]), len(ref.entries)
    dcomp = to_device(cref)
    buf = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for kw, bit in (({"out_capacity": need - 1}, 1), ({"out_capacity": need, "out_batch_capacity": nbat - 1}, 2)):
        got, dev = run_device(engine, dcomp, out_buffer=buf, **kw)
        assert int(got.totals["overflow"]) == bit
        assert int(got.totals["out_capacity_needed"]) == need
        assert int(got.totals["out_batch_capacity_needed"]) == nbat
        assert int(got.totals["batches_out"]) == nbat and int(got.totals["bytes_out"]) == need - 16
        assert bool(torch.all(buf == 0xA5)), "bytes written although a capacity was too small"
        assert not bool(torch.any(dev.entries)) and not bool(torch.any(dev.batches))
    # the needs reported: succeeds, and the guard behind the buffer stays
    got, _ = run_device(engine, dcomp, out_buffer=buf, out_capacity=need, out_batch_capacity=nbat)
    assert_model_parity(got, ref)
    assert bool(torch.all(buf[need:] == 0xA5))
    # the default capacities always suffice
    got, _ = run_device(engine, dcomp)
    assert_model_parity(got, ref)


@pytest.mark.gpu
def test_gpu_source_overflow(engine, oracle):
    """A compact call that itself overflowed: bit 2, nothing written, every offset 0."""
    import torch
    segs = [TC.tiny_segment(oracle)]
    _, cref, _, dcomp = TC.run_device(engine, oracle, segs, out_capacity=int(compact_need(oracle, segs)) - 1, sync=False)
    assert int(dcomp.totals_host()["overflow"]) & 1
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    got, dev = run_device(engine, dcomp, out_buffer=buf, out_capacity=4096, out_batch_capacity=8)
    assert int(got.totals["overflow"]) == 4
    assert int(got.totals["batches_out"]) == 0 and int(got.totals["bytes_out"]) == 0
    assert not np.any(got.out_seg_offsets) and bool(torch.all(buf == 0xA5))
    assert not bool(torch.any(dev.entries)) and not bool(torch.any(dev.batches))
    assert int(got.summaries[0]["n_batches"]) == 0


def compact_need(O, segs):
    return TC._ref_compact(O, segs)[0].totals["out_capacity_needed"]


@pytest.mark.gpu
def test_gpu_bad_codec_threshold_and_none(engine, oracle):
    from redpanda_amd._lib import RpgpuError
    pays = [bytes(139), bytes(138), bytes(140)]
    cref = laid_out(pays, [abi.CODEC_LZ4] * 3)
    dcomp = to_device(cref)
    for kw in ({"codec": 5}, {"min_batch_bytes": 200}, {"codec": abi.CODEC_NONE}, {"codec": abi.CODEC_GZIP},
               {"codec": abi.CODEC_SNAPPY, "min_batch_bytes": 201}):
        got, _ = run_device(engine, dcomp, **kw)
        assert_model_parity(got, RR.recompress(cref, **kw))
    got, _ = run_device(engine, dcomp, codec=5)
    assert np.all(got.entries["flags"] == abi.RECOMPRESS_F_BAD_CODEC) and np.all(got.entries["codec"] == 5)
    assert got.out.tobytes() == cref.out.tobytes()
    got, _ = run_device(engine, dcomp, min_batch_bytes=200)
    assert [int(f) for f in got.entries["flags"]] == [abi.RECOMPRESS_F_COMPRESSED, 0, abi.RECOMPRESS_F_COMPRESSED]
    with pytest.raises(RpgpuError):
        engine.recompress(dcomp, snappy_frag=100)
    with pytest.raises(RpgpuError):
        engine.recompress(dcomp, codec=8)
