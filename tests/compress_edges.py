"""Constructed payloads that put the block compressors (rp_compress.hip
lz4c_block / snappyc_block / wave_count / sn_copy / sn_literal, and their
mirror images in the device decoders) on the encoding edges of the two
formats, and the two parsers that prove each payload reaches its edge
(tests/test_compress_edges.py checks every claim against the oracle's output).

Every payload is a function of fixed parameters: nothing is searched at
import.  Random bytes come from 1..255, so a stretch of zeros is always a
separator that matches only itself.

cases()  -> [(name, bytes)], the edge in the name
claims() -> {name: (kind, ...)}, what the self-check must find in the
            oracle's encoding of that case

Run as a script, it prints what tests/compress_corpus.py and this corpus
reach of those edges, side by side (histogram()).
"""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------
# parsers
# ---------------------------------------------------------------------------
# one LZ4 sequence: literals block[lit_pos:lit_pos + lit_len], then match_len
# bytes from `offset` back; dst = the match's position in the decoded block
# (so its source is dst - offset).  The last sequence has no match (offset 0).
Seq = namedtuple("Seq", "lit_pos lit_len offset match_len dst")


def lz4_sequences(block):
    """The sequences of one LZ4 block (block format, not the frame)."""
    seqs, i, out, n = [], 0, 0, len(block)
    while True:
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        lp = i
        i += lit
        out += lit
        if i >= n:
            if i != n:
                raise ValueError("literals run past the block")
            seqs.append(Seq(lp, lit, 0, 0, out))
            return seqs
        off = block[i] | block[i + 1] << 8
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if off == 0 or off > out:
            raise ValueError(f"offset {off} at output {out}")
        seqs.append(Seq(lp, lit, off, ml, out))
        out += ml


def _copy_back(out, offset, length):
    src = len(out) - offset
    if offset >= length:
        out += out[src:src + length]
    else:
        pat = bytes(out[src:])
        out += (pat * (length // offset + 1))[:length]


def lz4_block_decode(block):
    """Decode through lz4_sequences (the parser used as the decoder)."""
    out = bytearray()
    for s in lz4_sequences(block):
        out += block[s.lit_pos:s.lit_pos + s.lit_len]
        assert len(out) == s.dst
        if s.offset:
            _copy_back(out, s.offset, s.match_len)
    return bytes(out)


def lz4_frame_blocks(frame):
    """[(raw?, block bytes)] of an LZ4 frame as lz4_frame_compressor writes it
    (no block or content checksums)."""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    i = 4 + 2 + (8 if frame[4] & 0x08 else 0) + 1
    blocks = []
    while True:
        w = int.from_bytes(frame[i:i + 4], "little")
        i += 4
        if w == 0:
            assert i == len(frame)
            return blocks
        n = w & 0x7FFFFFFF
        blocks.append((bool(w >> 31), frame[i:i + n]))
        i += n


def lz4_frame_decode(frame):
    return b"".join(b if raw else lz4_block_decode(b) for raw, b in lz4_frame_blocks(frame))


# one snappy element: kind "lit" (pos = where its bytes are in the stream),
# "copy1" (2-byte element, 11-bit offset, length 4..11) or "copy2" (3-byte
# element, 16-bit offset, length 1..64)
El = namedtuple("El", "kind length offset pos")


def snappy_elements(raw):
    """(uncompressed length, [El]) of a raw snappy stream."""
    i = ulen = shift = 0
    while True:
        b = raw[i]
        i += 1
        ulen |= (b & 0x7F) << shift
        shift += 7
        if b < 128:
            break
    els = []
    while i < len(raw):
        tag = raw[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                ln = int.from_bytes(raw[i:i + nb], "little")
                i += nb
            ln += 1
            els.append(El("lit", ln, 0, i))
            i += ln
        elif kind == 1:
            els.append(El("copy1", 4 + ((tag >> 2) & 7), (tag >> 5) << 8 | raw[i], 0))
            i += 1
        elif kind == 2:
            els.append(El("copy2", (tag >> 2) + 1, raw[i] | raw[i + 1] << 8, 0))
            i += 2
        else:
            raise ValueError("4-byte-offset copy: the compressor never writes one")
    if i != len(raw):
        raise ValueError("element runs past the stream")
    return ulen, els


def snappy_raw_decode(raw):
    ulen, els = snappy_elements(raw)
    out = bytearray()
    for e in els:
        if e.kind == "lit":
            out += raw[e.pos:e.pos + e.length]
        else:
            if e.offset == 0 or e.offset > len(out):
                raise ValueError(f"offset {e.offset} at output {len(out)}")
            _copy_back(out, e.offset, e.length)
    assert len(out) == ulen
    return bytes(out)


def snappy_java_chunks(frame):
    """The raw snappy streams of a snappy-java frame, one per fragment."""
    assert frame[:16] == b"\x82SNAPPY\x00\x01\x00\x00\x00\x01\x00\x00\x00"
    i, chunks = 16, []
    while i < len(frame):
        n = int.from_bytes(frame[i:i + 4], "big")
        chunks.append(frame[i + 4:i + 4 + n])
        i += 4 + n
    assert i == len(frame)
    return chunks


def snappy_java_decode(frame):
    return b"".join(snappy_raw_decode(c) for c in snappy_java_chunks(frame))


def snappy_chains(els):
    """[(output position, offset, [element lengths], [element kinds])]:
    consecutive copies with one offset are one match of the compressor, split
    by EmitCopy."""
    out, chains, prev = 0, [], None
    for e in els:
        if e.kind == "lit":
            prev = None
        elif prev is not None and prev[1] == e.offset:
            prev[2].append(e.length)
            prev[3].append(e.kind)
        else:
            prev = (out, e.offset, [e.length], [e.kind])
            chains.append(prev)
        out += e.length
    return chains


def lz4_probed(seqs):
    """Every position of the block that LZ4_compress_generic can have put in
    its hash table, from the sequences alone: position 0, the forward scan's
    probe positions after each anchor (its step schedule is fixed; it may
    have stopped earlier than the match start only if it never got there),
    and the two positions re-inserted after each match.  A match whose source
    is NOT in this set was found at a later position and extended backwards."""
    ins, anchor, first = {0}, 0, True
    for s in seqs:
        start = s.dst  # the match's start after the backward extension
        ip = 1 if first else anchor + 1
        if not first:
            ins.add(anchor)  # the immediate re-match probe
        first = False
        step, nb = 1, 64
        # the scan found its match at or after `start`, and within the match
        end = start + (s.match_len if s.offset else 0)
        while ip < end:
            ins.add(ip)
            ip += step
            step = nb >> 6
            nb += 1
        if s.offset:
            anchor = end
            ins.add(anchor - 2)
    return ins


def lz4_replay_exits(seqs, n, cap):
    """Which of LZ4_compress_generic's three limitedOutput checks stops the
    block at `cap` output bytes: 1 (before a literal run), 2 (after a match's
    length is known), 3 (the last literals), or 0 when it fits.  A sequence
    with no literals that came through the re-match path skips check 1; with
    lit_len 0 check 2 is never the weaker one, so it is skipped here too."""
    op = 0
    for s in seqs:
        if not s.offset:
            last = s.lit_len
            return 3 if op + last + 1 + (last + 240) // 255 > cap else 0
        op += 1
        if s.lit_len and op + s.lit_len + 8 + s.lit_len // 255 > cap:
            return 1
        if s.lit_len >= 15:
            op += (s.lit_len - 15) // 255 + 1
        op += s.lit_len + 2
        mc = s.match_len - 4
        if op + 6 + (mc + 240) // 255 > cap:
            return 2
        if mc >= 15:
            op += (mc - 15) // 255 + 1
    raise ValueError("no last sequence")


# ---------------------------------------------------------------------------
# payloads
# ---------------------------------------------------------------------------
_salt = 0  # the variant of the case being built (VARIANT)


def rnd(seed, n):
    """n bytes in 1..255"""
    return np.random.default_rng([seed, _salt]).integers(1, 256, n, dtype=np.uint8).tobytes()


def _differ(a, b):
    """b, its first byte changed if it equals a's first byte"""
    return b if a[0] != b[0] else bytes([(b[0] % 255) + 1]) + b[1:]


Z = b"\0"
LZ4_MATCH_LENGTHS = (4, 5, 18, 19, 20, 67, 68, 69, 131, 132, 133, 273, 274, 275, 528, 529, 530)
LIT_RUNS = (14, 15, 16, 269, 270, 271, 524, 525, 526)
SNAPPY_TOTALS = (4, 11, 12, 59, 60, 61, 63, 64, 65, 66, 67, 68, 69, 71, 72, 127, 128, 129, 131, 132, 133)
SNAPPY_LITS = (59, 60, 61, 255, 256, 257)


def lz4_match(L):
    """zeros, then A .. A with exactly L equal bytes: the bytes before and
    after the two copies differ.  The zeros keep the block compressible, so a
    4-byte match is not lost to a raw block."""
    a, sep, tail = rnd(1000 + L, L), rnd(2000 + L, 20), rnd(3000 + L, 16)
    pre = rnd(4000 + L, 8)
    sep = sep[:-1] + bytes([(pre[-1] % 255) + 1])  # no backward extension past A
    tail = _differ(sep, tail)
    return Z * 64 + pre + a + sep + a + tail


def lz4_literals(k):
    """match, exactly k literals, match: M g M lit(k) M tail"""
    m, g, lit, tail = rnd(5000 + k, 16), rnd(5100 + k, 6), rnd(5200 + k, k), rnd(5300 + k, 16)
    lit = _differ(g, lit)
    lit = lit[:-1] + bytes([(g[-1] % 255) + 1])
    tail = _differ(lit, _differ(g, tail))
    if tail[0] == g[0]:
        tail = bytes([(tail[0] % 255) + 1]) + tail[1:]
    return Z * 32 + b"\x01" + m + g + m + lit + m + tail


def lz4_rematch():
    """A x B y A B: the match of A ends where B begins, and B is in the table"""
    a, b = rnd(5400, 16), rnd(5401, 16)
    x, y, tail = _differ(b, rnd(5402, 4)), rnd(5403, 8), rnd(5404, 16)
    return Z * 32 + b"\x01" + a + x + b + y + a + b + tail


def lz4_last_literals(k):
    a, g = rnd(5500 + k, 24), rnd(5600 + k, 6)
    return Z * 32 + b"\x01" + a + g + a + _differ(g, rnd(5700 + k, k))


def lz4_back_to_zero(gap):
    """A at block byte 0 and again after `gap` literals: the scan, by then in
    steps of 2, finds the second copy one byte late and walks back to match
    position 0, where only the `match > 0` guard stops it."""
    a = rnd(5800, 40)
    return a + rnd(5801, gap) + a + rnd(5802, 16)


def lz4_back_to_anchor(u):
    """200 literals (the scan is in steps of 2 and 3 at their end, so position
    u there is never inserted), a run of zeros (a match: a fresh anchor), then
    the 24 bytes at u again: the re-match probe at the anchor misses, the scan
    finds u + 1 one byte later and walks back to the anchor."""
    p = rnd(5900, 200)
    return p + Z * 40 + p[u:u + 24] + rnd(5901, 16)


def lz4_far_offset():
    """a 65536-byte block: 20 bytes at position 1, zeros, and the 20 bytes
    again at 65510 (offset 65509, the match ends 6 bytes before the block
    does).  65535 itself cannot be reached inside one block: the source would
    be byte 0 and the match would start at 65535, past the last position
    (n - 12) at which the compressor looks for one."""
    a = rnd(6000, 20)
    s = b"\x01" + a + Z * 65486 + rnd(6001, 3) + a + rnd(6002, 6)
    assert len(s) == 65536
    return s


def lz4_exit_literals():
    """64 KiB of random bytes and, in the last 160, two copies of bytes 2..62
    (the scan's steps are near 45 by then; a shorter repeat is stepped over):
    the literal run in front of the match no longer fits, check 1"""
    a = bytearray(rnd(6100, 65536))
    for q in (65380, 65445):
        a[q:q + 60] = a[2:62]
    return bytes(a)


def lz4_exit_match(P):
    """P random bytes, a 104-byte copy from inside them, a 12-byte tail: check 2"""
    a = rnd(5, P)
    return a + a[1000:1104] + rnd(6, 12)


def lz4_fit(reps, seed):
    """3000 random bytes with `reps` planted 4-byte repeats 12 bytes apart
    (the literals between them need no length byte): each saves a byte"""
    a = bytearray(rnd(seed, 3000))
    for i in range(reps):
        q = 100 + 12 * i
        a[q:q + 4] = a[q - 6:q - 2]
    return bytes(a)


def snappy_copy(T, zeros, tail=16):
    """x A g zeros A tail: the zeros are a match of their own, so the second A
    is probed at its first byte with a fresh skip, and A (at position 1: snappy
    never inserts position 0) is copied whole: total T, offset T + 1 + zeros."""
    a, t = rnd(7000 + T + zeros, T), rnd(7100 + T, tail)
    g = bytes([(t[0] % 255) + 1])
    return b"\x01" + a + g + Z * zeros + a + t


def snappy_tail_literal(k):
    a = rnd(7200 + k, 16)
    g = rnd(7300 + k, 2)
    return b"\x01" + a + g + Z * 40 + a + _differ(g, rnd(7400 + k, k))


def snappy_mid_literal(k):
    """m, zeros (a match: the skip is fresh after it), k literals, m again; k
    is an offset that the scan probes (1..33, then every 2nd: 35, 37, ...; 60
    and 255..257 are not, those lengths are reached as a block's last literal)"""
    m = rnd(7500 + k, 12)
    return b"\x01" + m + b"\x02" + Z * 40 + rnd(7600 + k, k) + m + rnd(7700 + k, 16)


def _build():
    out, claims = [], {}

    def add(name, build, *claim):
        global _salt
        assert name not in claims
        _salt = VARIANT.get(name, 0)
        out.append((name, build() if callable(build) else build))
        claims[name] = claim

    # ---- LZ4 ----
    for L in LZ4_MATCH_LENGTHS:
        add(f"lz4_match_{L}", lambda: lz4_match(L), "lz4_match", L, L + 20)
    for n in range(77, 141):
        add(f"lz4_mlimit_run_{n}", b"x" * n, "lz4_mlimit")
    pat = rnd(4500, 150)
    for m in range(80, 144):
        add(f"lz4_mlimit_copy_{m}", pat + pat[:m], "lz4_mlimit")
    add("lz4_literals_0_rematch", lz4_rematch, "lz4_literals", 0)
    for k in LIT_RUNS:
        add(f"lz4_literals_{k}", lambda: lz4_literals(k), "lz4_literals", k)
    for k in LIT_RUNS:
        add(f"lz4_last_literals_{k}", lambda: lz4_last_literals(k), "lz4_last_literals", k)
    add("lz4_back_to_anchor", lambda: lz4_back_to_anchor(BACK_TO_ANCHOR_U), "lz4_back_to_anchor")
    add("lz4_back_to_byte0", lambda: lz4_back_to_zero(BACK_TO_ZERO_GAP), "lz4_back_to_byte0", 40 + BACK_TO_ZERO_GAP)
    add("lz4_offset_1", b"a" * 300, "lz4_offset", 1, 1, 200)
    add("lz4_offset_2", b"ab" * 200, "lz4_offset", 2, 2, 200)
    add("lz4_offset_3", b"abc" * 150, "lz4_offset", 3, 3, 200)
    add("lz4_offset_65509", lz4_far_offset, "lz4_offset", 65509, 65509, 20)
    add("lz4_exit1_literal_run", lz4_exit_literals, "lz4_exit", 1)
    add("lz4_exit2_match_length", lambda: lz4_exit_match(EXIT2_P), "lz4_exit", 2)
    add("lz4_exit3_last_literals", lambda: rnd(6200, 1000), "lz4_exit", 3)
    add("lz4_fits_n_minus_1", lambda: lz4_fit(*FIT_N_MINUS_1), "lz4_size", -1)
    add("lz4_raw_at_n", lambda: lz4_fit(*FIT_N), "lz4_size", 0)

    # ---- snappy ----
    for T in sorted(set(SNAPPY_TOTALS) | set(range(4, 12))):
        add(f"snappy_copy_{T}", lambda: snappy_copy(T, 40), "snappy_copy", T, T + 41)
    for T in range(4, 12):
        add(f"snappy_copy_{T}_far", lambda: snappy_copy(T, 2100), "snappy_copy", T, T + 2101)
    for off in (2047, 2048):
        add(f"snappy_copy_8_offset_{off}", lambda: snappy_copy(8, off - 9), "snappy_copy", 8, off)
    add("snappy_copy_20_offset_65121", lambda: snappy_copy(20, 65100), "snappy_copy", 20, 65121)
    for k in SNAPPY_LITS:
        add(f"snappy_literal_{k}", lambda: snappy_tail_literal(k), "snappy_literal", k)
    for k in SNAPPY_MID_LITS:
        add(f"snappy_literal_{k}_before_copy", lambda: snappy_mid_literal(k), "snappy_literal", k)
    add("snappy_literal_whole_block", lambda: rnd(7800, 3000), "snappy_literal", 3000)
    for n in range(70, 134):
        add(f"snappy_end_run_{n}", b"x" * n, "snappy_end")
    for m in range(80, 144):
        add(f"snappy_end_copy_{m}", pat + pat[:m], "snappy_end")
    blk = (rnd(7900, 251) * 262)[:65536]
    add("snappy_second_block_9", blk + rnd(7901, 9), "snappy_blocks", 9)
    t = rnd(7902, 60)
    add("snappy_second_block_140", blk + t + rnd(7903, 20) + t, "snappy_blocks", 140)
    return out, claims


# found once on the CPU (see each builder's docstring), fixed here
BACK_TO_ANCHOR_U = 151
BACK_TO_ZERO_GAP = 61
EXIT2_P = 26805
FIT_N_MINUS_1 = (14, 6300)
FIT_N = (13, 6300)
SNAPPY_MID_LITS = (59, 61)
# cases whose first variant of random bytes missed the edge by a chance
# collision in the hash table: the variant that hits
VARIANT = {"snappy_copy_9": 1, "snappy_copy_61": 1}

_built = None


def cases():
    """[(name, bytes)]"""
    global _built
    if _built is None:
        _built = _build()
    return list(_built[0])


def claims():
    cases()
    return dict(_built[1])


def histogram(lz4_blocks, snappy_streams):
    """What a corpus reaches, from the oracle's output: lz4_blocks
    [(raw?, block)], snappy_streams [raw stream].  Printed by running this
    file, for tests/compress_corpus.py and for this corpus."""
    h = {"lz4 raw blocks": 0, "lz4 matches >= 68 ended by a mismatch": 0, "lz4 matches >= 68 ended by mlimit": 0,
         "lz4 match lengths 273..275": 0, "lz4 literal runs 269..271 / 524..526": 0, "lz4 literal runs >= 270": 0,
         "lz4 max offset": 0, "lz4 offsets >= 65000": 0, "lz4 offsets 1..3 with length >= 68": 0,
         "snappy copy totals 60..140": 0, "snappy literals 256 / 257": 0, "snappy copies < 12 at offset < 2048": 0,
         "snappy copies < 12 at offset >= 2048": 0, "snappy max offset": 0}
    for raw, block in lz4_blocks:
        if raw:
            h["lz4 raw blocks"] += 1
            continue
        seqs = lz4_sequences(block)
        n = seqs[-1].dst
        for s in seqs:
            h["lz4 literal runs 269..271 / 524..526"] += s.lit_len in (269, 270, 271, 524, 525, 526)
            h["lz4 literal runs >= 270"] += s.lit_len >= 270
            if not s.offset:
                continue
            by_limit = s.dst + s.match_len == n - 5
            h["lz4 matches >= 68 ended by mlimit"] += s.match_len >= 68 and by_limit
            h["lz4 matches >= 68 ended by a mismatch"] += s.match_len >= 68 and not by_limit
            h["lz4 match lengths 273..275"] += s.match_len in (273, 274, 275)
            h["lz4 max offset"] = max(h["lz4 max offset"], s.offset)
            h["lz4 offsets >= 65000"] += s.offset >= 65000
            h["lz4 offsets 1..3 with length >= 68"] += s.offset <= 3 and s.match_len >= 68
    for raw in snappy_streams:
        _, els = snappy_elements(raw)
        h["snappy literals 256 / 257"] += sum(1 for e in els if e.kind == "lit" and e.length in (256, 257))
        for _, off, lens, _ in snappy_chains(els):
            t = sum(lens)
            h["snappy copy totals 60..140"] += 60 <= t <= 140
            h["snappy copies < 12 at offset < 2048"] += t < 12 and off < 2048
            h["snappy copies < 12 at offset >= 2048"] += t < 12 and off >= 2048
            h["snappy max offset"] = max(h["snappy max offset"], off)
    return h


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import compress_corpus
    from oracle import oracle as O
    rows = []
    for corpus, frags in ((compress_corpus.cases(), compress_corpus.FRAGS), (cases(), (0, 4097))):
        blocks = [b for _, d in corpus for b in lz4_frame_blocks(O.compress(3, d, 0))]
        streams = [c for _, d in corpus for f in frags for c in snappy_java_chunks(O.compress(2, d, f))]
        rows.append(histogram(blocks, streams))
    print(f"{'':48}{'compress_corpus':>16}{'compress_edges':>16}")
    for k in rows[0]:
        print(f"{k:48}{rows[0][k]:>16}{rows[1][k]:>16}")
