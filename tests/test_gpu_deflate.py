"""gzip compression on the device (rpgpu_set_device_gzip; k_deflate,
rp_deflate.hip): rpgpu_compress_batch's gzip payloads against the golden
vectors of zlib 1.2.11 (tests/golden/gzip_compress_vectors.json, made on the
CPU from Python's zlib; tests/test_deflate_core.py pins the host build of the
same text against the library itself).  Every comparison is exact, and the
GPU machine's own libz is not relied on: the switch-off comparison is made
against the same vectors."""
import hashlib
import json
import os

import numpy as np
import pytest

import batchgen as BG
import compress_corpus as CC
import gzip_compress_corpus as G
from redpanda_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "gzip_compress_vectors.json")))["vectors"]

pytestmark = pytest.mark.gpu


def _digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()]


@pytest.fixture(scope="module")
def named():
    return G.named_cases()


@pytest.fixture()
def gz(engine):
    """the session's engine with the switch on for the length of one test"""
    engine.set_device_gzip(True)
    yield engine
    engine.set_device_gzip(False)


@pytest.fixture(scope="module")
def frames(engine, named):
    """every named case at every fragment size, compressed on the device in
    one call: {name/frag: bytes}; also checks the payload counter"""
    keys, pays, frags = [], [], []
    for name, data in named:
        for frag in G.FRAGS:
            keys.append(f"{name}/{frag}")
            pays.append(data)
            frags.append(frag)
    engine.set_device_gzip(True)
    try:
        before = engine.gzip_device_payloads()
        res = engine.compress_batch([abi.CODEC_GZIP] * len(pays), pays, frags)
        assert engine.gzip_device_payloads() - before == len(pays)
    finally:
        engine.set_device_gzip(False)
    assert all(st == 0 for st, _ in res)
    return {k: f for k, (_, f) in zip(keys, res)}


def test_device_gzip_matches_golden(frames):
    assert len(frames) == len(GOLD)
    bad = [k for k, f in frames.items() if _digest(f) != GOLD[k]]
    assert not bad, bad


def test_device_frames_decode_on_device(engine, named, frames):
    """the frames, as gzip batches of one segment, through the device's gzip
    decoder in a CRC | DECODE job"""
    pays = [(n, d) for n, d in named if len(d)]
    seg = b"".join(BG.batch(frames[f"{n}/4096"], 1, base_offset=i, attrs=abi.CODEC_GZIP)
                   for i, (n, d) in enumerate(pays))
    data = np.frombuffer(seg, dtype=np.uint8)
    import torch
    got = engine.validate(torch.from_numpy(data.copy()).cuda(), [0, data.size], abi.JOB_CRC | abi.JOB_DECODE,
                          decoded_capacity=sum(len(d) + 64 for _, d in pays) + (1 << 16))
    assert len(got.batches) == len(pays)
    for (name, d), b in zip(pays, got.batches):
        assert int(b["flags"]) & abi.F_CODEC_OK, name
        o, n = int(b["decoded_off"]), int(b["decoded_len"])
        assert n == len(d) and got.decoded[o:o + n].tobytes() == d, name


def test_switch_off_same_bytes_counter_still(engine, named):
    """off (the default): the host path; the counter does not move.  The
    bytes are compared with the golden vectors where the host's libz gives
    zlib 1.2.11's bytes, and decode back in any case."""
    import zlib
    sample = [(n, d) for n, d in named if n in ("len0", "text40", "abcabcabc", "rand20000", "text65274", "fib20")]
    before = engine.gzip_device_payloads()
    res = engine.compress_batch([abi.CODEC_GZIP] * len(sample), [d for _, d in sample], [1000] * len(sample))
    assert engine.gzip_device_payloads() == before
    for (name, d), (st, f) in zip(sample, res):
        assert st == 0 and zlib.decompress(f, 31) == d, name
        if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":
            assert _digest(f) == GOLD[f"{name}/1000"], name


def test_overflow_reports_exact_size(gz, named, frames):
    data = dict(named)["json100k"]
    full = frames["json100k/4096"]
    (st, need), (st1, exact) = gz.compress_batch([abi.CODEC_GZIP] * 2, [data, data], [4096, 4096],
                                                 caps=[len(full) - 1, len(full)])
    assert st == abi.E_OVERFLOW and need == len(full)
    assert st1 == 0 and exact == full


def test_mixed_codecs_one_call(gz, oracle):
    """LZ4, snappy and gzip payloads (and a host zstd one) in one call"""
    from oracle import oracle as O
    pays = [CC.text(70_000, 1), CC.json_like(30_000, 2), dict(G.named_cases())["text65536"], CC.low_entropy(5000, 3),
            dict(G.named_cases())["rand20000"], b"x" * 10]
    codecs = [abi.CODEC_LZ4, abi.CODEC_SNAPPY, abi.CODEC_GZIP, abi.CODEC_SNAPPY, abi.CODEC_GZIP, abi.CODEC_ZSTD]
    frags = [0, 1001, 65280, 0, 0, 0]
    before = gz.gzip_device_payloads()
    res = gz.compress_batch(codecs, pays, frags)
    assert gz.gzip_device_payloads() - before == 2
    assert [st for st, _ in res] == [0] * 6
    for i in (0, 1, 3):
        assert res[i][1] == O.compress(codecs[i], pays[i], frags[i]), i
    assert _digest(res[2][1]) == GOLD["text65536/65280"]
    assert _digest(res[4][1]) == GOLD["rand20000/0"]


@pytest.mark.parametrize("count,lo,hi", [(256, 1000, 40_000), (1100, 200, 3000)])
def test_work_list_cursor(gz, count, lo, hi):
    """256 payloads of 1-40 KB, and more payloads (1100) than resident
    streams (1024), so that waves take a second payload from the list.  The
    expectation is the host build of the same core, which the CPU tests pin
    against zlib 1.2.11."""
    import zlib
    from redpanda_amd import build as B
    from test_deflate_core import load_host
    host = load_host(B.build_deflate_host())
    rng = np.random.default_rng(count)
    makers = [CC.text, CC.json_like, CC.low_entropy, CC.mostly_random]
    pays = [makers[i % 4](int(rng.integers(lo, hi + 1)), 500 + i) for i in range(count)]
    frags = [0 if i % 3 else 777 for i in range(count)]
    before = gz.gzip_device_payloads()
    res = gz.compress_batch([abi.CODEC_GZIP] * count, pays, frags)
    assert gz.gzip_device_payloads() - before == count
    for i, ((st, f), d) in enumerate(zip(res, pays)):
        assert st == 0 and f == host(d, frags[i]), i
        assert zlib.decompress(f, 31) == d, i
        if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":  # independent of the core, where the library is the pinned one
            c = zlib.compressobj(-1, zlib.DEFLATED, 31, 8, 0)
            step = frags[i] or len(d)
            assert f == b"".join(c.compress(d[k:k + step]) for k in range(0, len(d), step)) + c.flush(), i
