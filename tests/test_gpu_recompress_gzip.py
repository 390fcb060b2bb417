"""rpgpu_recompress with rpgpu_set_device_gzip on: the gzip batches of a
compacted job are compressed where they lie (k_deflate_blocks), one fragment
each, and nothing is left for the host.  The expectation is
tests/recompress_ref.py's model with the gzip batches compressed too: by the
host build of rp_deflate_core.h, which tests/test_deflate_core.py pins against
zlib 1.2.11, and which is compared with Python's zlib here wherever that is
1.2.11.  Every comparison is exact."""
import zlib

import numpy as np
import pytest

from redpanda_amd import abi
from tests import batchgen as BG
from tests import compress_corpus as CC
from tests import recompress_ref as RR
from tests import test_recompress as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gzip_one_fragment():
    from redpanda_amd import build as B
    from tests.test_deflate_core import load_host
    host = load_host(B.build_deflate_host())

    def gz(raw):
        out = host(raw, 0)
        if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":
            c = zlib.compressobj(-1, zlib.DEFLATED, 31, 8, 0)
            assert out == c.compress(raw) + c.flush()
        return out
    return gz


def compacted():
    """three small segments (3 + 2 + 3 batches) of one-record batches: gzip,
    LZ4 and uncompressed entries; payloads from 80 bytes to past the second
    window slide, text, random (a stored block) and a long run"""
    vals = [CC.text(300, 1), CC.json_like(70_000, 2), CC.random_bytes(5000, 3), CC.text(140_000, 4), b"z" * 40,
            b"\x05" * 100_000, CC.low_entropy(9000, 5), CC.text(20, 6)]
    codecs = [abi.CODEC_GZIP, abi.CODEC_LZ4, abi.CODEC_GZIP, abi.CODEC_GZIP, abi.CODEC_NONE, abi.CODEC_GZIP,
              abi.CODEC_LZ4, abi.CODEC_GZIP]
    pays = [BG.record(0, b"key%d" % i, v) for i, v in enumerate(vals)]
    return TR.laid_out(pays, codecs, seg_counts=[3, 2, 3])


def model(cref, gz):
    """recompress_ref.recompress(cref) with the RECOMPRESS_F_HOST gzip batches
    finished as the device finishes them: compressed, attrs |= gzip, stamped"""
    from oracle import oracle as O
    base = RR.recompress(cref)
    out, positions, plens = bytearray(), [], []
    entries = base.entries.copy()
    seg_off = np.zeros_like(base.out_seg_offsets)
    s = 0
    for i, e in enumerate(base.entries):
        p, n = int(e["out_pos"]), int(e["payload_len"])
        while s < len(seg_off) - 1 and p >= int(base.out_seg_offsets[s]):
            seg_off[s] = len(out)
            s += 1
        hdr, pay = bytearray(base.out[p:p + 61].tobytes()), base.out[p + 61:p + 61 + n].tobytes()
        flags = int(e["flags"])
        if flags & abi.RECOMPRESS_F_HOST and int(e["codec"]) == abi.CODEC_GZIP:
            pay = gz(pay)
            hdr[21] |= abi.CODEC_GZIP
            flags = abi.RECOMPRESS_F_COMPRESSED
        if flags & abi.RECOMPRESS_F_COMPRESSED:
            positions.append(len(out))
            plens.append(len(pay))
        entries[i]["out_pos"], entries[i]["payload_len"], entries[i]["flags"] = len(out), len(pay), flags
        out += bytes(hdr) + pay
    while s < len(seg_off):
        seg_off[s] = len(out)
        s += 1
    buf = O.stamp_batches(np.frombuffer(bytes(out) + b"\0" * 16, dtype=np.uint8), positions, plens, 0, abi.STAMP_CRC)
    data = np.array(buf[:len(out)])
    tot = base.totals.copy()
    tot["batches_compressed"] = len(positions)
    tot["batches_host"] = 0
    tot["bytes_out"] = len(out)
    tot["out_capacity_needed"] = len(out) + 16
    job = O.run_job(data, seg_off, abi.JOB_CRC)
    return RR.RefRecompress(data, seg_off, entries, job.batches, job.summaries, tot, job)


@pytest.fixture(scope="module")
def chain(engine, oracle, gzip_one_fragment):
    cref = compacted()
    ref = model(cref, gzip_one_fragment)
    dcomp = TR.to_device(cref)
    engine.set_device_gzip(True)
    try:
        got, dev = TR.run_device(engine, dcomp)
    finally:
        engine.set_device_gzip(False)
    return dict(cref=cref, ref=ref, dcomp=dcomp, got=got, dev=dev)


def test_gzip_batches_compressed_in_place(chain):
    got, ref = chain["got"], chain["ref"]
    TR.assert_model_parity(got, ref)
    assert int(got.totals["batches_host"]) == 0
    assert int(got.totals["batches_compressed"]) == 7
    gz = got.entries[got.entries["codec"] == abi.CODEC_GZIP]
    assert len(gz) == 5 and set(int(f) for f in gz["flags"]) == {abi.RECOMPRESS_F_COMPRESSED}
    for e in gz:
        p, n = int(e["out_pos"]), int(e["payload_len"])
        raw = zlib.decompress(got.out[p + 61:p + 61 + n].tobytes(), 31)
        assert len(raw) == int(e["in_payload_len"])


def test_output_validates_and_indexes(engine, oracle, chain):
    """a disk-layout CRC | PARSE | DECODE job over the output; rpgpu_segment_index over d_out_batches"""
    TR.assert_closure(engine, oracle, chain["got"], chain["ref"], TR.compact_payloads(chain["cref"]), parse=True)
    TR.assert_index(engine, oracle, chain["dev"], chain["ref"])


def test_switch_off_leaves_gzip_to_the_host(engine, chain):
    got, _ = TR.run_device(engine, chain["dcomp"])
    TR.assert_model_parity(got, RR.recompress(chain["cref"]))
    assert int(got.totals["batches_host"]) == 5


def test_out_capacity_one_byte_short(engine, chain):
    import torch
    ref = chain["ref"]
    need = int(ref.totals["out_capacity_needed"])
    buf = torch.full((need + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    engine.set_device_gzip(True)
    try:
        got, dev = TR.run_device(engine, chain["dcomp"], out_buffer=buf, out_capacity=need - 1)
        assert int(got.totals["overflow"]) == 1
        assert int(got.totals["out_capacity_needed"]) == need
        assert bool(torch.all(buf == 0xAA)), "bytes written although out_capacity was too small"
        assert not bool(torch.any(dev.entries)) and not bool(torch.any(dev.batches))
        got, _ = TR.run_device(engine, chain["dcomp"], out_buffer=buf, out_capacity=need)
        TR.assert_model_parity(got, ref)
        assert bool(torch.all(buf[need:] == 0xAA))
    finally:
        engine.set_device_gzip(False)
