"""The CRC32C stream geometry of every kernel that calls crc_stream
(rp_validate.hip): k_validate in disk and wire layout, k_stamp and
k_validate_decoded, bit-exact against the CPU oracle on payloads placed at
every window / head / injection / tail situation (tests/crc_geometry.py).
k_crc_split and k_crc_compose have their cases in tests/diag_cases.py.

The tests without the gpu mark assert, with the CPU model geom(), that the
case sets reach what they claim, that the oracle accepts every clean batch
and no corrupted twin, and that on the tiny set the pure-Python CRC of
tests/batchgen.py agrees with the oracle's.
"""
import os
import sys

import numpy as np
import pytest

from redpanda_amd import abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchgen as BG  # noqa: E402
import crc_geometry as CG  # noqa: E402

WIN = CG.WIN
FLAGS = abi.JOB_CRC | abi.JOB_PARSE
DFLAGS = FLAGS | abi.JOB_DECODE
CLEAN = ("A", "B", "C", "D")


class Sets:
    """The clean segments A..D, then the twins of A, of every eighth batch of
    B, and of C, as the segments of one job."""

    def __init__(self, O):
        self.seg, self.cases = {}, {}
        self.seg["A"], self.cases["A"] = CG.build(O, CG.cases_a(), 0xA)
        self.seg["B"], self.cases["B"] = CG.build(O, CG.cases_b(), 0xB)
        self.seg["C"], self.cases["C"] = CG.build(O, CG.cases_c(), 0xC)
        self.seg["D"], self.cases["D"] = CG.build(O, CG.cases_d(), 0xD, payload=CG.payload_d)
        self.hit, self.zone = {}, {}
        for k, every in (("A", 1), ("B", 8), ("C", 1)):
            self.seg["t" + k], self.hit["t" + k], self.zone["t" + k] = CG.twins(self.seg[k], self.cases[k], every)
        self.names = list(CLEAN) + ["tA", "tB", "tC"]
        self.segs = [self.seg[k] for k in self.names]
        self.offs = np.cumsum([0] + [s.size for s in self.segs]).astype(np.uint64)
        self._ref = {}
        self.O = O

    def geoms(self, name):
        """geom() of every case of a clean set, at its place in the job."""
        base = int(self.offs[self.names.index(name)])
        return [CG.geom(base + c.S, base + c.S + c.n) for c in self.cases[name]]

    def ref(self, flags, layout=abi.LAYOUT_DISK, names=None):
        key = (flags, layout, names)
        if key not in self._ref:
            self._ref[key] = run_oracle(self.O, self.job(names, layout)[0], flags, layout)
        return self._ref[key]

    def job(self, names=None, layout=abi.LAYOUT_DISK):
        segs = [self.seg[k] for k in (names or self.names)]
        if layout == abi.LAYOUT_WIRE:
            segs = [np.frombuffer(BG.disk_to_wire(s.tobytes()), dtype=np.uint8) for s in segs]
        return segs, np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)


def run_oracle(O, segs, flags, layout=abi.LAYOUT_DISK):
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    total = int(offs[-1])
    return O.run_job(np.concatenate(segs), offs, flags, layout=layout, record_cap=max(total // 7, 64),
                     decoded_cap=max(total * 2, 1 << 16) if flags & abi.JOB_DECODE else 1 << 16)


_SETS = []


@pytest.fixture(scope="module")
def sets(oracle):
    if not _SETS:
        _SETS.append(Sets(oracle))
    return _SETS[0]


def batch_index(res, seg, pos):
    """Ordinals of the batches of segment `seg` whose headers sit at `pos`."""
    b = res.batches
    of = np.flatnonzero(b["segment"] == seg)
    at = np.searchsorted(b["file_pos"][of], np.asarray(pos, dtype=np.uint64))
    assert np.array_equal(b["file_pos"][of][at], np.asarray(pos, dtype=np.uint64))
    return of[at]


# ---------------------------------------------------------------------------
# the model, and what the case sets reach
# ---------------------------------------------------------------------------
def test_geom_model_by_hand():
    g = CG.geom
    assert g(0, 0) == (0, 0, 0, None, 0)
    assert g(5, 5) == (0, 1, 5, None, 0)
    assert g(3, 14) == (0, 3, 3, None, 11)            # inside one row: all tail
    assert g(3, 16) == (1, 3, 3, WIN - 12, 0)         # E16 = 16: the window is [16 - 16K, 16), S4 = 4
    assert g(16, 35) == (1, 0, 0, WIN - 16, 3)
    assert g(13, 16) == (1, 1, 13, WIN, 0)            # S4 = 16 = E16: the window holds no word of the stream
    assert g(13, 21) == (1, 1, 13, WIN, 5)
    assert g(0, WIN) == (1, 0, 0, 0, 0)               # window 0 starts exactly at S
    assert g(0, WIN + 16) == (2, 0, 0, WIN - 16, 0)
    assert g(16, 2 * WIN + 16 + 7) == (2, 0, 0, 0, 7)
    assert g(13, WIN + 16) == (2, 1, 13, WIN, 0)      # E16 - S = 16K + 3: window 0 holds 3 head bytes only
    assert g(1, 3 * WIN + 12) == (3, 1, 1, 4, 12)     # E16 = 3 * 16K: window 0 starts at 0, S4 = 4


def test_segments_keep_their_geometry(sets):
    for s in sets.segs:
        assert s.size % 16 == 0
    for k in ("A", "B", "C"):
        assert sets.seg["t" + k].size == sets.seg[k].size


def test_set_a_reaches_every_tiny_case(sets):
    gs = sets.geoms("A")
    cs = sets.cases["A"]
    assert {(g.s16, c.n) for g, c in zip(gs, cs)} == {(s, n) for s in range(16) for n in range(41)}
    # no window: every start and end inside the tail row
    assert {(g.s16, g.s16 + c.n) for g, c in zip(gs, cs) if g.R == 0} >= \
        {(s, e) for s in range(16) for e in range(s, 16)}
    assert any(c.n == 0 for c in cs)
    # the one-window stream whose injection point is the window's end
    assert {g.s4 for g in gs if g.R == 1 and g.o4 == WIN} == {1, 2, 3}
    assert {g.tail for g in gs if g.R == 1 and g.o4 == WIN} == set(range(16))


def test_set_b_reaches_every_injection_offset(sets):
    gs = sets.geoms("B")
    assert all(g.R == 1 for g in gs)
    assert {g.o4 for g in gs} == set(range(0, WIN + 1, 4))
    cs = sets.cases["B"]
    assert {(g.s16, (g.s16 + c.n) % 16) for g, c in zip(gs, cs)} == {(s, e) for s in range(16) for e in range(16)}


def test_set_c_reaches_every_window_count(sets):
    gs = sets.geoms("C")
    cs = sets.cases["C"]
    assert {(g.s16, c.n) for g, c in zip(gs, cs)} == \
        {(s, WIN * m + d) for m in (1, 2, 3) for d in range(-20, 41) for s in CG.C_STARTS}
    assert {g.R for g in gs} == {1, 2, 3, 4}
    # the injection point at the end of window 0 of a multi-window stream, for every head length
    for R in (2, 3, 4):
        assert {g.s4 for g in gs if g.R == R and g.o4 == WIN} == {1, 2, 3}
    # window 0 starting exactly at S
    assert {g.R for g in gs if g.o4 == 0 and g.s16 == 0} == {1, 2, 3}


def test_set_d_is_walked_by_k_validate(sets):
    gs = sets.geoms("D")
    cs = sets.cases["D"]
    n0 = min(c.n for c in cs)
    assert {(g.s16, c.n) for g, c in zip(gs, cs)} == {(s, n0 + k) for s in range(16) for k in range(CG.D_WIDTH)}
    assert all(g.R == 1 for g in gs)
    ref = sets.ref(FLAGS)
    i = batch_index(ref, sets.names.index("D"), [c.pos for c in cs])
    assert np.all(ref.batches["record_count"][i] == CG.D_RECORDS) and CG.D_RECORDS > 256  # kLaneWalkMax
    assert np.all(ref.batches["flags"][i] & abi.F_PARSE_OK)


def test_twins_flip_every_zone(sets):
    for k in ("tA", "tC"):
        assert set(sets.zone[k]) == set(range(6))
        assert len(sets.hit[k]) >= len(sets.cases[k[1]]) - 16     # all but the empty payloads
    assert set(sets.zone["tB"]) == set(range(6))
    assert len(sets.hit["tB"]) >= len(sets.cases["B"]) // 8
    for k in ("A", "B", "C"):
        d = np.flatnonzero(sets.seg[k] != sets.seg["t" + k])
        assert len(d) == len(sets.hit["t" + k])                   # one byte per twin, each inside its payload
        lo = np.array([c.S for c in sets.hit["t" + k]])
        hi = np.array([c.S + c.n for c in sets.hit["t" + k]])
        assert np.all((d >= lo) & (d < hi))


def test_oracle_accepts_clean_and_rejects_twins(sets):
    ref = sets.ref(FLAGS)
    b = ref.batches
    ok = (b["flags"] & abi.F_CRC_OK) != 0
    assert np.all((b["flags"] & abi.F_HEADER_OK) != 0)
    for k in CLEAN:
        of = b["segment"] == sets.names.index(k)
        assert np.sum(of) >= len(sets.cases[k]) and np.all(ok[of]), k
    for k in ("tA", "tB", "tC"):
        seg = sets.names.index(k)
        bad = batch_index(ref, seg, [c.pos for c in sets.hit[k]])
        assert not np.any(ok[bad]), k
        rest = np.setdiff1d(np.flatnonzero(b["segment"] == seg), bad)
        assert np.all(ok[rest]), k
    # every payload with 8 bytes or more is well-formed records (one, or two where no single record fits)
    for k in ("A", "B", "C"):
        i = batch_index(ref, sets.names.index(k), [c.pos for c in sets.cases[k] if c.n >= 8])
        assert np.all(b["flags"][i] & abi.F_PARSE_OK) and np.all(b["records_parsed"][i] == b["record_count"][i]), k
        assert np.all(b["record_count"][i] >= 1) and np.sum(b["record_count"][i] != 1) <= 4, k


def test_set_a_crc_by_pure_python(sets):
    """tests/batchgen.py's table CRC, independent of the oracle's C one."""
    seg = sets.seg["A"].tobytes()
    for c in sets.cases["A"]:
        (_, size, _, _, crc, attrs, lod, first, mx, pid, epoch, seq, rc) = BG.DISK_HDR.unpack_from(seg, c.pos)
        assert size == CG.HDR + c.n
        want = BG.crc32c(seg[c.S:c.S + c.n], BG.crc32c(BG.be_prefix(attrs, lod, first, mx, pid, epoch, seq, rc)))
        assert crc & 0xFFFFFFFF == want, c


def test_diag_jobs_reach_their_cases(oracle):
    """The jobs of the crc_split_small and crc_compose_small cases
    (tests/diag_cases.py, run on the GPU by tests/test_gpu_diag.py): the
    builders assert by the model what the split parts and the gaps reach; the
    oracle rejects the twins and nothing else."""
    from tests import diag_cases as D
    segs, twins = D.split_small_job(oracle)
    b = run_oracle(oracle, segs, FLAGS).batches
    assert int(np.sum((b["flags"] & abi.F_CRC_OK) == 0)) == twins == len(D.SPLIT_GROUPS)
    assert int(np.sum(b["size_bytes"] - abi.HEADER_SIZE >= 1024)) == sum(len(ns) + 1 for ns in D.SPLIT_GROUPS)
    seg, eligible = D.compose_small_job(oracle)
    assert eligible == D.COMPOSE_ELIGIBLE and sum(eligible) > 0
    b = run_oracle(oracle, [seg], DFLAGS).batches
    assert list(np.flatnonzero((b["flags"] & abi.F_CRC_OK) == 0)) == D.COMPOSE_BAD_CRC


# ---------------------------------------------------------------------------
# GPU parity
# ---------------------------------------------------------------------------
def run_gpu(engine, segs, ref, flags, chunk=0, layout=abi.LAYOUT_DISK):
    import torch
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    data = np.concatenate(segs + [np.zeros(16, np.uint8)])
    d = torch.from_numpy(data).cuda()[: data.size - 16]
    return engine.validate(d, offs, flags, chunk_bytes=chunk, layout=layout,
                           batch_capacity=len(ref.batches) + 16, record_capacity=len(ref.records) + 64)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 4096])
@pytest.mark.parametrize("flags", [abi.JOB_CRC, FLAGS], ids=["crc", "crc_parse"])
def test_gpu_disk_layout(engine, sets, flags, chunk):
    """k_validate over A..D and the twins: crc_computed is compared too, so a
    twin must show the oracle's wrong value, not just a cleared flag."""
    from test_gpu_parity import assert_same
    ref = sets.ref(flags)
    got = run_gpu(engine, sets.segs, ref, flags, chunk)
    assert_same(got, ref, flags)
    assert "crc_computed" in abi.BATCH_COMPARE_FIELDS
    assert int(got.totals["reserved"][0]) == 0 and int(got.totals["reserved"][1]) == 0  # the product build reports no counts


WIRE = ("A", "C", "D", "tA")


@pytest.mark.gpu
def test_gpu_wire_layout(engine, sets):
    """The same payloads as Kafka record sets (writer_serialize_batch keeps
    the 61-byte header, so every S mod 16 stays)."""
    from test_gpu_parity import assert_same
    segs, _ = sets.job(WIRE, abi.LAYOUT_WIRE)
    for s, k in zip(segs, WIRE):
        assert s.size == sets.seg[k].size
    ref = sets.ref(FLAGS, abi.LAYOUT_WIRE, WIRE)
    assert len(ref.batches) >= sum(len(sets.cases[k]) for k in ("A", "C", "D", "A"))
    ok = (ref.batches["flags"] & abi.F_CRC_OK) != 0
    assert np.all(ok[ref.batches["segment"] < 3]) and not np.all(ok[ref.batches["segment"] == 3])
    got = run_gpu(engine, segs, ref, FLAGS, layout=abi.LAYOUT_WIRE)
    assert_same(got, ref, FLAGS)


@pytest.mark.gpu
def test_gpu_stamp(engine, sets):
    """k_stamp: the clean A + B + C with header_crc, size_bytes and crc
    blanked comes back byte-identical, and equal to the oracle's stamp."""
    import torch
    from test_stamp import CRC, blank
    names = ("A", "B", "C")
    segs, offs = sets.job(names)
    data = np.concatenate(segs)
    ref = sets.ref(abi.JOB_CRC, names=names)
    b = ref.batches
    pos = (b["file_pos"] + offs[b["segment"]]).astype(np.uint64)
    pl = (b["size_bytes"] - abi.HEADER_SIZE).astype(np.uint32)
    assert len(pos) >= sum(len(sets.cases[k]) for k in names)
    z = blank(data, pos, offsets=False)
    assert not np.array_equal(z, data)
    want = sets.O.stamp_batches(z, pos, pl, 0, CRC)
    np.testing.assert_array_equal(want, data)
    d = torch.from_numpy(np.concatenate([z, np.zeros(16, np.uint8)])).cuda()
    engine.stamp(d, pos, pl, 0, CRC)
    got = d[: data.size].cpu().numpy()
    np.testing.assert_array_equal(got, data)


# ---------------------------------------------------------------------------
# k_validate_decoded: arena slots are 16-byte aligned, so only the decoded
# length matters
# ---------------------------------------------------------------------------
def snappy_literals(plain: bytes) -> bytes:
    """Raw snappy of literal elements only (format_description.txt: the
    varint length, then tag 00 literals of up to 64 KiB here)."""
    out = bytearray()
    n = len(plain)
    while True:
        out.append((n & 0x7F) | (0x80 if n >= 0x80 else 0))
        n >>= 7
        if not n:
            break
    for a in range(0, len(plain), 60000):
        lit = plain[a:a + 60000]
        m = len(lit) - 1
        if m < 60:
            out.append(m << 2)
        elif m < 256:
            out += bytes([60 << 2, m])
        else:
            out += bytes([61 << 2, m & 0xFF, m >> 8])
        out += lit
    return bytes(out)


RAW_LENS = list(range(1101)) + [1024 * k + d for k in range(1, 17) for d in (0, 4, 15, 16, 17)] + \
    [WIN * m + d for m in (1, 2) for d in range(-20, 37)]
CODEC_LENS = list(range(49)) + [WIN + d for d in range(-20, 37)]


def decoded_segments(O):
    from gzip_corpus import gzip_member
    import zstd_corpus as ZC
    rng = np.random.default_rng(0xDEC)
    enc = [("raw", abi.CODEC_SNAPPY, snappy_literals, RAW_LENS),
           ("java", abi.CODEC_SNAPPY, lambda p: O.compress(abi.CODEC_SNAPPY, p), CODEC_LENS),
           ("gzip", abi.CODEC_GZIP, lambda p: gzip_member(p, 6), CODEC_LENS),
           ("zstd", abi.CODEC_ZSTD, lambda p: ZC.frame(p), CODEC_LENS),
           ("lz4", abi.CODEC_LZ4, lambda p: O.compress(abi.CODEC_LZ4, p), CODEC_LENS)]
    segs, lens = [], []
    for _, codec, f, ns in enc:
        out = bytearray()
        for i, n in enumerate(ns):
            plain, rc = CG.payload_of(n, rng)
            pay = f(plain)
            ts = 1600000000000
            crc = O.crc32c(pay, O.crc32c(BG.be_prefix(codec, rc - 1, ts, ts + max(rc - 1, 0), -1, -1, -1, rc)))
            out += BG.batch(pay, rc, base_offset=i, attrs=codec, crc=crc)
        segs.append(np.frombuffer(bytes(out), dtype=np.uint8).copy())
        lens.append(ns)
    return segs, lens


@pytest.mark.gpu
def test_gpu_decoded_lengths(engine, oracle):
    """decoded_crc, decoded_header_crc and the arena of payloads whose decoded
    length takes every value around the row, window and tail edges."""
    from test_gpu_parity import assert_same
    segs, lens = decoded_segments(oracle)
    ref = run_oracle(oracle, segs, DFLAGS)
    b = ref.batches
    assert len(b) == sum(len(n) for n in lens)
    assert np.all(b["flags"] & abi.F_CRC_OK) and np.all(b["flags"] & abi.F_CODEC_OK)
    np.testing.assert_array_equal(b["decoded_len"], np.concatenate([np.asarray(n) for n in lens]))
    assert np.all(b["decoded_off"] % 16 == 0)
    got = run_gpu(engine, segs, ref, DFLAGS)
    for f in ("decoded_crc", "decoded_header_crc", "decoded_len", "decoded_off"):
        np.testing.assert_array_equal(got.batches[f], b[f], err_msg=f)
    assert_same(got, ref, DFLAGS)
