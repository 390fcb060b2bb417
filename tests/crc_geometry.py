"""Batches aimed at the geometry of crc_stream (redpanda_amd/csrc/
rp_validate.hip), and a CPU model of that geometry.

crc_stream cuts a payload [S, E) of the job buffer into 16 KiB windows
anchored at E16 = E & ~15: window 0 may begin before S, up to 3 head bytes
before the first 4-aligned position S4 are folded in from a scalar load, the
running state is injected at word offset o4 of window 0 (rows and words before
it masked), and the 0..15 bytes [E16, E) follow as the tail.  A payload inside
one 16-byte row has no window (R == 0), and S4 can land exactly on the end of
window 0 (o4 == WIN).  geom() restates that arithmetic; the case sets below
place payloads so that every one of those situations occurs, and
tests/test_crc_geometry.py asserts with geom() that they do.

Batches are built with tests/batchgen.py; the batch crc is the oracle's C
crc32c (the pure-Python one is too slow for the larger sets, and is compared
with it on set A).  A payload of n >= 8 bytes is one well-formed record whose
value fills it (two records at the two lengths no single record has), so the
walks see the same alignments; smaller ones are raw bytes with record_count 0.  A segment
holds no gaps, so tiny filler batches steer the next payload's S mod 16, and
every segment ends on a multiple of 16: a copy of a segment anywhere in a job
keeps its geometry.
"""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchgen as BG  # noqa: E402

WIN = 16384   # kWinBytes
HDR = 61      # RPGPU_HEADER_SIZE (disk and wire headers alike)

Geom = namedtuple("Geom", "R s4 s16 o4 tail")
Case = namedtuple("Case", "pos S n")   # header position, payload start and length within the segment


def geom(S: int, E: int) -> Geom:
    """(R, S % 4, S % 16, o4 or None, tail_len) of the stream [S, E):
    make_stream / win_base and the S4, o4 arithmetic of crc_stream."""
    E16 = E & ~15
    R = (E16 - S + WIN - 1) // WIN if E16 > S else 0
    o4 = None
    if R:
        S4 = (S + 3) & ~3
        o4 = S4 - (E16 - WIN * R)
    return Geom(R, S % 4, S % 16, o4, E - max(S, E16))


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def _vlen(v: int) -> int:
    return len(BG.vint(v))


def one_record(n: int, rng, i: int = 0):
    """One well-formed record of exactly n >= 8 bytes whose value fills it (a
    null key, or a one-byte key where the value's length varint grows), or
    None: no record is 65 or 8194 bytes long (the record length varint grows
    by a byte there)."""
    for key in (None, b"k"):
        kb = 1 + (len(key) if key else 0)            # key length varint + key
        for lv in (1, 2, 3, 4):                      # bytes of the record length varint
            body = n - lv
            for vv in (1, 2, 3, 4):                  # bytes of the value length varint
                vl = body - 3 - kb - vv - 1          # attrs, ts, offset deltas; headers count
                if vl >= 0 and _vlen(vl) == vv and _vlen(body) == lv:
                    r = BG.record(i, key, rng.bytes(vl) if vl else b"")
                    assert len(r) == n
                    return r
    return None


def payload_of(n: int, rng):
    """(payload, record_count) of n bytes: one record, or a minimal record and
    a second one at the two lengths no single record has."""
    if n < 8:
        return rng.bytes(n), 0
    r = one_record(n, rng)
    if r is not None:
        return r, 1
    return BG.record(0, None, b"") + one_record(n - 7, rng, 1), 2


class Segment:
    """A disk segment under construction at a 16-aligned place of a job."""

    def __init__(self, O, seed: int):
        self.O = O
        self.rng = np.random.default_rng(seed)
        self.buf = bytearray()
        self.cases = []
        self.base = 0

    def _emit(self, payload: bytes, count: int) -> int:
        lod = count - 1
        ts = 1600000000000
        crc = self.O.crc32c(payload, self.O.crc32c(BG.be_prefix(0, lod, ts, ts + max(count - 1, 0), -1, -1, -1, count)))
        pos = len(self.buf)
        self.buf += BG.batch(payload, count, base_offset=self.base, crc=crc)
        self.base += max(count, 1)
        return pos

    def steer(self, s16: int):
        """A filler batch of 0..15 raw bytes so that the next payload starts
        at s16 mod 16 (none when it already would)."""
        f = (s16 - (len(self.buf) + HDR) - HDR) % 16
        if (len(self.buf) + HDR) % 16 != s16 % 16:
            self._emit(self.rng.bytes(f), 0)
        assert (len(self.buf) + HDR) % 16 == s16 % 16

    def add(self, s16: int, n: int, payload=None, count=None):
        self.steer(s16)
        if payload is None:
            payload, count = payload_of(n, self.rng)
        pos = self._emit(payload, count)
        self.cases.append(Case(pos, pos + HDR, n))

    def finish(self):
        """-> (segment bytes as uint8, [Case]); the length a multiple of 16."""
        if len(self.buf) % 16:
            self._emit(self.rng.bytes((-(len(self.buf) + HDR)) % 16), 0)
        assert len(self.buf) % 16 == 0
        return np.frombuffer(bytes(self.buf), dtype=np.uint8).copy(), self.cases


# ---------------------------------------------------------------------------
# case lists: (S mod 16, n)
# ---------------------------------------------------------------------------
def cases_a():
    """Tiny: every (S mod 16, n), n in 0..40."""
    return [(s, n) for n in range(41) for s in range(16)]


def cases_b():
    """Injection offset: one-window payloads with every 4-aligned o4 in
    [0, WIN], and every pair (S mod 16, E mod 16)."""
    out = []
    for k in range(WIN // 4 + 1):
        o4 = 4 * k
        # S4 = o4 (mod 16): the four starts that round up to it
        starts = [(o4 - d) % 16 for d in (0, 1, 2, 3)]
        if o4 == 0:
            starts = starts[:1]      # window 0 starts exactly at S
        if o4 == WIN:
            starts = starts[1:]      # E16 - S in {1, 2, 3}
        j = k // 4
        s = starts[j % len(starts)]
        t = (j // 4) % 16
        head = (-s) % 4
        out.append((s, WIN - o4 + head + t))
    return out


C_STARTS = (0, 1, 2, 3, 4, 8, 12, 13, 14, 15)


def cases_c():
    """Window count: n in 16384 m + [-20, +40], m in {1, 2, 3}."""
    return [(s, WIN * m + d) for m in (1, 2, 3) for d in range(-20, 41) for s in C_STARTS]


D_RECORDS = 257
D_WIDTH = 64


def cases_d():
    """In-kernel walk: 64 consecutive lengths, each at every S mod 16."""
    return [(s, k) for k in range(D_WIDTH) for s in range(16)]


def payload_d(k: int, rng):
    """257 records (more than k_walk takes), 256 minimal ones and a last one
    whose value is padded by k bytes."""
    recs = [BG.record(i & 63, None, b"") for i in range(D_RECORDS - 1)]
    recs.append(one_record(66 + k, rng))  # (past the one length below it that no record has)
    p = b"".join(recs)
    assert len(p) == 7 * (D_RECORDS - 1) + 66 + k
    return p, D_RECORDS


def build(O, cases, seed, payload=None):
    """Segment of the (S mod 16, n) cases; `payload(n, rng)` overrides
    payload_of (its n is then whatever the case list means by it)."""
    seg = Segment(O, seed)
    for s, n in cases:
        if payload is None:
            seg.add(s, n)
        else:
            p, c = payload(n, seg.rng)
            seg.add(s, len(p), p, c)
    return seg.finish()


# ---------------------------------------------------------------------------
# corrupted twins
# ---------------------------------------------------------------------------
def zones(S: int, n: int):
    """Byte positions of the six flip zones of the payload [S, S + n), None
    where it has no such zone: the first byte, the last head byte before S4,
    the first word at o4, byte E16 - 1, byte E16, byte E - 1."""
    E = S + n
    g = geom(S, E)
    E16, S4 = E & ~15, (S + 3) & ~3
    return [S if n else None,
            S4 - 1 if g.R and S4 != S else None,
            S4 if g.R and S4 < E else None,
            E16 - 1 if g.R else None,
            E16 if E > E16 >= S else None,
            E - 1 if n else None]


def twins(seg: np.ndarray, cases, every: int = 1):
    """A copy of `seg` with one payload bit flipped in every `every`-th case,
    cycling through the zones (skipping those a payload lacks).  -> (segment,
    [Case] of the flipped batches, [zone index] of each)."""
    out = seg.copy()
    hit, which = [], []
    z = 0
    for i, c in enumerate(cases[::every]):
        zs = zones(c.S, c.n)
        if not any(p is not None for p in zs):
            continue  # the empty payload
        while zs[z % 6] is None:
            z += 1
        out[zs[z % 6]] ^= 1 << (i % 8)
        hit.append(c)
        which.append(z % 6)
        z += 1
    return out, hit, which
