"""Cases that need the diagnostic library variant (librpgpu_diag.so, built by
__graft_entry__.build(); environment overrides of pool sizes and of the host
codec's availability).  A process loads one librpgpu, so tests/test_gpu_diag.py
runs each case here in a child process with RPGPU_VARIANT=diag:

    python -m tests.diag_cases <case>

exit status 0 = the case held; anything else prints why.
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from redpanda_amd import abi  # noqa: E402

DFLAGS = abi.JOB_CRC | abi.JOB_PARSE | abi.JOB_DECODE


def _gzip_payloads():
    """Clean gzip members of several sizes plus members whose ISIZE trailer
    claims ~4 GiB (the first pass's slot guess is payload-controlled)."""
    from tests import batchgen as BG
    from tests.gzip_corpus import gzip_member
    good = [gzip_member(BG.simple_records(n, vlen=v, seed=n), 6, 0) for n, v in
            [(5, 20), (40, 100), (300, 400), (900, 900), (60, 2000)]]
    hostile = []
    for p in good[1:4]:
        q = bytearray(p)
        q[-4:] = struct.pack("<I", 0xFFFFFFF0)
        hostile.append(bytes(q))
    return good[:2] + hostile[:1] + good[2:] + hostile[1:] + good


def case_small_pool():
    """RPGPU_INF_POOL_KIB=64: most members get no first-pass slot (and the
    hostile ISIZE ones are capped), so they decode in the second pass; every
    output is still the oracle's."""
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests.test_gpu_parity import _gzip_batches, assert_same, run_both
    assert os.environ.get("RPGPU_INF_POOL_KIB"), "run with RPGPU_INF_POOL_KIB"
    O.build()
    eng = Engine(0)
    pay = _gzip_payloads()
    segs = [_gzip_batches(pay), _gzip_batches(pay[::-1], base=5000)]
    got, ref = run_both(eng, O, segs, flags=DFLAGS)
    ok = (got.batches["flags"] & abi.F_CODEC_OK) != 0
    assert int(np.sum(ok)) >= 2 * 8, int(np.sum(ok))
    assert_same(got, ref, DFLAGS)
    print(f"small_pool ok: {len(got.batches)} batches, {int(np.sum(ok))} decoded")


def case_host_codec_missing():
    """RPGPU_HOST_CODEC_MISSING=1: with RPGPU_JOB_HOST_CODECS a job holding
    zstd batches fails with RPGPU_E_UNSUPPORTED (valid payloads are never
    reported corrupt); without the flag the device decodes them."""
    import torch
    from oracle import oracle as O
    from redpanda_amd._lib import RpgpuError
    from redpanda_amd.engine import Engine
    from tests.test_gpu_parity import assert_same, gen, run_both
    assert os.environ.get("RPGPU_HOST_CODEC_MISSING") == "1"
    O.build()
    eng = Engine(0)
    segs = [gen(None, 1 << 20, i, seed=0x2E0 + i, batch_bytes=0, min_batch=200, max_batch=200000,
                weights=[1, 0, 0, 1, 3, 0]) for i in range(2)]
    data = np.concatenate(segs)
    offs = np.cumsum([0] + [s.size for s in segs]).astype(np.uint64)
    d = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()[: data.size]
    try:
        eng.validate(d, offs, DFLAGS | abi.JOB_HOST_CODECS)
    except RpgpuError as e:
        assert f"[{abi.E_UNSUPPORTED}]" in str(e), e
    else:
        raise AssertionError("a host-codec job without libzstd must fail with RPGPU_E_UNSUPPORTED")
    got, ref = run_both(eng, O, segs, flags=DFLAGS)
    assert np.any(((got.batches["attrs"] & 7) == abi.CODEC_ZSTD) & ((got.batches["flags"] & abi.F_CODEC_OK) != 0))
    assert_same(got, ref, DFLAGS)
    print("host_codec_missing ok")


def case_small_frec():
    """RPGPU_FREC_CAP=n: the fast-path record pool holds n records, so the
    planner lists the first groups of LZ4 blocks for k_lzf_walk and leaves
    every later group (note_fast: no room) to k_lz_walk / k_lz_exec; frames
    mix listed blocks with walked ones.  Every field is still the oracle's
    (rp_codec.hip note_fast)."""
    import random
    import synth
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests import test_gpu_lz4_walk as W
    from tests.test_gpu_parity import assert_same, gen, run_both
    assert os.environ.get("RPGPU_FREC_CAP"), "run with RPGPU_FREC_CAP"
    O.build()
    eng = Engine(0)
    rnd = random.Random(11)
    frames = []
    for kind in ("mixed", "text", "long_lits", "long_match"):
        for _ in range(3):
            blk, _ = W.valid_block(rnd, kind)
            frames.append(W.frame([blk]))
    for _ in range(3):  # several blocks per frame, so a frame's blocks can land on both sides of the cut
        blks = [W.valid_block(rnd, "text") for _ in range(4)]
        frames.append(W.frame([b for b, _ in blks]))
        frames.append(W.frame([b for b, _ in blks], content=b"".join(o for _, o in blks)))
    frames += W.raw_block_frames(rnd)
    frames += [W.frame([b]) for b in W.bad_blocks(rnd)]
    rnd.shuffle(frames)
    segs = [W.segment(frames[i::2]) for i in range(2)]
    kw = dict(synth.C2, lz4_linked_ppm=200000, lz4_content_checksum_ppm=200000, lz4_block_checksum_ppm=50000)
    segs += [gen(None, 6 << 20, i, **kw) for i in range(2)]
    got, ref = run_both(eng, O, segs, flags=DFLAGS)
    ok = (ref.batches["flags"] & abi.F_CODEC_OK) != 0
    assert int(np.sum(ok)) > len(frames) // 2
    assert_same(got, ref, DFLAGS)
    print(f"small_frec ok: {len(got.batches)} batches, {int(np.sum(ok))} decoded")


def case_zstd_ring_wave():
    """RPGPU_ZS_FAST=0: every zstd member through the wave decoder (ZDev, no
    lane parser), so the ring-mode members it turns down reach k_zexact from
    k_members_first rather than from k_zfallback; libzstd's bytes either way."""
    import random
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests import zstd_corpus as ZC
    from tests.test_gpu_parity import _zstd_batches, assert_same, run_both
    assert os.environ.get("RPGPU_ZS_FAST") == "0"
    O.build()
    eng = Engine(0)
    rng = random.Random(7)
    frames = ZC.ring_frames(rng, 80)
    pay = [f for _, f in frames] + ZC.mutations(rng, frames[:10], per=3)
    got, ref = run_both(eng, O, [_zstd_batches(pay, counts=[1] * len(pay))], flags=DFLAGS)
    ok = (ref.batches["flags"] & abi.F_CODEC_OK) != 0
    assert int(np.sum(ok)) >= 40, int(np.sum(ok))
    assert_same(got, ref, DFLAGS)
    print(f"zstd_ring_wave ok: {len(got.batches)} batches, {int(np.sum(ok))} decoded")


PATH_SWITCHES = ("RPGPU_XXH_SIDE", "RPGPU_CRC_COMPOSE", "RPGPU_DCHAIN", "RPGPU_GZS", "RPGPU_LZF")


def case_path_switch():
    """One of PATH_SWITCHES set to 0: the alternative path it selects
    (content checksums inside k_decode_finish, k_validate streaming every
    stored payload, k_validate_decoded chaining the records itself, every gzip
    member serial, every LZ4 piece through the walk / exec kernels) gives the
    oracle's results on a small job of every codec."""
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests.test_gpu_parity import assert_same, gen, run_both
    off = [k for k in PATH_SWITCHES if os.environ.get(k) == "0"]
    assert len(off) == 1, f"run with exactly one of {PATH_SWITCHES} set to 0"
    O.build()
    eng = Engine(0)
    segs = [gen(None, 1 << 20, i, seed=0x5A0 + i, batch_bytes=0, min_batch=200, max_batch=200000,
                weights=[2, 2, 2, 4, 2, 2], lz4_content_checksum_ppm=300000, lz4_linked_ppm=300000,
                corrupt_payload_ppm=(30000 if i == 1 else 0)) for i in range(2)]
    got, ref = run_both(eng, O, segs, flags=DFLAGS)
    codec = ref.batches["attrs"] & 7
    ok = (ref.batches["flags"] & abi.F_CODEC_OK) != 0
    for cd in (abi.CODEC_GZIP, abi.CODEC_SNAPPY, abi.CODEC_LZ4, abi.CODEC_ZSTD):
        assert np.any(ok & (codec == cd)), f"no decoded batch of codec {cd}"
    assert_same(got, ref, DFLAGS)
    if off[0] == "RPGPU_CRC_COMPOSE":
        assert diag_counts(got)[1] == 0, diag_counts(got)
    print(f"path_switch {off[0]}=0 ok: {len(got.batches)} batches, {int(np.sum(ok))} decoded")


def diag_counts(res):
    """(payloads k_validate listed for k_crc_split, crcs k_crc_compose stored):
    rpgpu_job_totals.reserved[0] of the diagnostic build (k_finalize_totals)."""
    r = int(res.totals["reserved"][0])
    assert int(res.totals["reserved"][1]) == 0
    return r & 0xFFFFFFFF, r >> 32


SPLIT_GROUPS = (range(1024, 1024 + 272), range(262144 - 40, 262144 + 41), range(524288 - 40, 524288 + 41))


def split_small_job(O):
    """-> (segments, number of twins): payloads of 1024..1295 bytes and
    around 256 KiB and 512 KiB at cycling S mod 16, the last batch of each
    group a corrupted twin of its middle length.  Asserts, by the CPU model of
    tests/crc_geometry.py over the 16 parts of every payload (split_cut,
    rp_validate.hip: cuts at multiples of 16), what the parts reach."""
    from tests import crc_geometry as CG
    segs, parts, twins = [], [], 0
    for gi, ns in enumerate(SPLIT_GROUPS):
        cases = [((i // 16 + 3 * i) % 16, n) for i, n in enumerate(ns)]
        cases.append(cases[len(cases) // 2])
        seg, cs = CG.build(O, cases, 0x5B0 + gi)
        t = cs[-1]
        seg[t.S + (t.n * 5) // 8] ^= 0x04
        twins += 1
        base = sum(s.size for s in segs)
        segs.append(seg)
        for c in cs:
            cut = [c.n if k >= 16 else (c.n * k // 16) & ~15 for k in range(17)]
            g = [CG.geom(base + c.S + cut[k], base + c.S + cut[k + 1]) for k in range(16)]
            if gi == 0:
                assert {cut[k + 1] - cut[k] for k in range(15)} <= {64, 80}
            parts += g
    assert {g.tail for g in parts} == set(range(16)) and {g.s16 for g in parts} == set(range(16))
    assert {g.R for g in parts} == {1, 2, 3}
    assert {g.s4 for g in parts if g.R >= 2 and g.o4 == CG.WIN} == {1, 2, 3}
    return segs, twins


def case_crc_split_small():
    """RPGPU_SPLIT_MIN_KIB=1: every stored payload of 1 KiB or more goes
    through k_crc_split / k_crc_combine.  Payloads of 1024..1295 bytes (parts
    of 64 or 80 bytes, every tail length) and payloads around 256 KiB and
    512 KiB (parts crossing from one window to two and from two to three), one
    corrupted twin per group: the oracle's results, and the split count is the
    number of payloads of 1 KiB or more."""
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests.test_gpu_parity import FLAGS, assert_same, run_both
    assert os.environ.get("RPGPU_SPLIT_MIN_KIB") == "1"
    O.build()
    segs, twins = split_small_job(O)
    eng = Engine(0)
    got, ref = run_both(eng, O, segs, flags=FLAGS)
    b = ref.batches
    ok = (b["flags"] & abi.F_CRC_OK) != 0
    assert int(np.sum(~ok)) == twins, int(np.sum(~ok))
    assert_same(got, ref, FLAGS)
    want = int(np.sum(b["size_bytes"] - abi.HEADER_SIZE >= 1024))
    assert want == sum(len(ns) + 1 for ns in SPLIT_GROUPS)
    assert diag_counts(got) == (want, 0), (diag_counts(got), want)
    print(f"crc_split_small ok: {len(b)} batches, split count {want}, {twins} twins")


def lz4f_plan(p: bytes):
    """The blocks [(raw, size)] of an LZ4F payload that is complete in
    structure, else None; and whether its raw blocks are k_raw_copy's
    (independent blocks, no block checksum): plan_lz4f (rp_codec.hip)."""
    import xxhash
    n = len(p)
    if n < 7 or p[:4] != b"\x04\x22\x4d\x18":
        return None
    flg, bd = p[4], p[5]
    hsize = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if n < hsize or flg & 2 or (flg >> 6) & 3 != 1 or bd & 0x8F or (bd >> 4) & 7 < 4:
        return None
    if (xxhash.xxh32(p[4:hsize - 1], seed=0).intdigest() >> 8) & 0xFF != p[hsize - 1]:
        return None
    linked, bcs, ccs = not flg & 0x20, bool(flg & 0x10), bool(flg & 4)
    bmax = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}[(bd >> 4) & 7]
    pos, blocks, end = hsize, [], False
    while n - pos >= 4:
        bh = int.from_bytes(p[pos:pos + 4], "little")
        pos += 4
        if bh == 0:
            end = True
            break
        bsz = bh & 0x7FFFFFFF
        if bsz > bmax or n - pos < bsz + (4 if bcs else 0):
            return None
        pos += bsz + (4 if bcs else 0)
        blocks.append((bool(bh >> 31), bsz))
    if not end:
        return None
    if ccs:
        if n - pos < 4:
            return None
        pos += 4
    if pos != n or not blocks or (linked and len(blocks) > 64):
        return None
    return blocks, not bcs and not linked


def compose_raw_bytes(p: bytes):
    """Bytes of the payload's raw blocks that k_raw_copy copies (0: none)."""
    plan = lz4f_plan(p)
    return sum(sz for raw, sz in plan[0] if raw) if plan and plan[1] else 0


COMPOSE_ELIGIBLE = [True] * 15 + [False, False, True, True, False, True]
COMPOSE_BAD_CRC = [17, 18, 19]


def compose_small_job(O):
    """-> (segment, eligible flag per batch): LZ4F frames of two 64 KiB raw
    blocks around one literal-only compressed block.  Batches 0..12: the gap
    between the raw blocks (size word + block + size word) takes 58..70 bytes,
    both sides of gap()'s 64-byte short path; 13: a gap above 16 KiB with a
    tail; 14: a content checksum after the end mark; 15: trailing bytes after
    the end mark and 16: block checksums (neither composed); 17..19: twins of
    20 with a bit flipped in a raw block, in the gap and in a size word (the
    last no longer a frame); eligibility by the rules of k_crc_compose
    (rp_validate.hip: raw blocks at least half of the job; a payload of
    kComposeMin or more with raw blocks at least 3/4 of it)."""
    import random
    from tests import batchgen as BG
    from tests import test_gpu_lz4_walk as W
    rnd = random.Random(0xC0)

    def rawb():
        return rnd.randbytes(65536)

    def lits(ll):
        return W.seq(rnd.randbytes(ll))  # token + one length byte + the literals

    frames, gaps = [], []
    for gap in range(58, 71):
        c = lits(gap - 8 - 2)
        frames.append(W.frame([rawb(), c, rawb()], raw=(0, 2)))
        gaps.append(4 + len(c) + 4)
    big = lits(16384 + 777)
    frames.append(W.frame([rawb(), big, rawb()], raw=(0, 2)))
    gaps.append(4 + len(big) + 4)
    r0, lit, r1 = rawb(), rnd.randbytes(40), rawb()
    frames.append(W.frame([r0, W.seq(lit), r1], raw=(0, 2), content=r0 + lit + r1))
    frames.append(W.frame([rawb(), lits(51), rawb()], raw=(0, 2)) + b"trailing")
    frames.append(W.frame([rawb(), lits(52), rawb()], raw=(0, 2), bcs=True))
    base = W.frame([rawb(), lits(53), rawb()], raw=(0, 2))
    stored = [(f, f) for f in frames]
    for at in (7 + 4 + 30000, 7 + 4 + 65536 + 4 + 20, 7 + 1):  # raw block 0, the compressed block, block 0's size word
        t = bytearray(base)
        t[at] ^= 0x10
        stored.append((bytes(t), base))
    stored.append((base, base))
    assert gaps[:13] == list(range(58, 71)) and gaps[13] > 16384 + 16 and (gaps[13] + 7 + 4) % 16
    out = bytearray()
    ts = 1600000000000
    for k, (p, of) in enumerate(stored):  # a twin keeps the crc of the frame it was made from
        crc = O.crc32c(of, O.crc32c(BG.be_prefix(W.LZ4, 2, ts, ts + 2, -1, -1, -1, 3)))
        out += BG.batch(p, 3, base_offset=3 * k, attrs=W.LZ4, crc=crc)
    seg = np.frombuffer(bytes(out), dtype=np.uint8).copy()
    raw = [compose_raw_bytes(p) for p, _ in stored]
    assert sum(raw) and 2 * sum(raw) >= seg.size, "raw blocks under half of the job: k_crc_compose would return"
    return seg, [len(p) >= (64 << 10) and 4 * r >= 3 * len(p) for (p, _), r in zip(stored, raw)]


def case_crc_compose_small():
    """k_crc_compose at small shapes (compose_small_job): the oracle's
    results, crc_computed of the twins included, and k_crc_compose stored
    exactly the eligible frames' crcs."""
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests.test_gpu_parity import assert_same, run_both
    assert os.environ.get("RPGPU_CRC_COMPOSE") != "0"
    O.build()
    seg, eligible = compose_small_job(O)
    assert eligible == COMPOSE_ELIGIBLE, eligible
    eng = Engine(0)
    got, ref = run_both(eng, O, [seg], flags=DFLAGS)
    b = ref.batches
    assert len(b) == len(eligible)
    ok = (b["flags"] & abi.F_CRC_OK) != 0
    assert list(np.flatnonzero(~ok)) == COMPOSE_BAD_CRC, np.flatnonzero(~ok)
    assert np.sum((b["flags"] & abi.F_CODEC_OK) != 0) >= sum(eligible) - 1
    assert_same(got, ref, DFLAGS)
    want = sum(eligible)
    assert diag_counts(got) == (0, want), (diag_counts(got), want)
    print(f"crc_compose_small ok: {len(b)} batches, compose count {want}")


CASES = {"small_pool": case_small_pool, "host_codec_missing": case_host_codec_missing, "small_frec": case_small_frec,
         "zstd_ring_wave": case_zstd_ring_wave, "path_switch": case_path_switch,
         "crc_split_small": case_crc_split_small, "crc_compose_small": case_crc_compose_small}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
