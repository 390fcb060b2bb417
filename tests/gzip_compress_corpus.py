"""Deterministic payloads for the gzip compressor (rp_deflate_core.h, the
device's k_deflate): the named edge cases of zlib 1.2.11's deflate at level 6
(named_cases(), at most 300 KB each: what the golden vectors and the GPU
tests use), the payloads of compress_corpus.py (cases()), and seeded random
inputs with random fragmentations (random_inputs()).

Why each named case is there:
  len0..len263        the empty stream; inputs below MIN_MATCH; the lookahead
                      around MIN_LOOKAHEAD (262)
  far32506/7, far32768  a 64-byte string whose only earlier copy lies at that
                      distance: MAX_DIST is 32506, so the first is a match and
                      the others are literals
  text65273..65277    strstart reaches w_size + MAX_DIST (65274): the first slide
  text65535..65537    the window fills exactly (window_size 65536)
  text131069..131075  the second fill / slide
  rand20000           more than 16383 symbols (two blocks), both stored
  text40              a fixed block beats a dynamic one
  run300k, period8    blocks far longer than the window: block_start has slid
                      out (negative), a stored block is impossible
  toofar4096/4097     a 3-byte match at distance 4096 is kept, at 4097 dropped
  abcabcabc           window position 0 is NIL: never a match candidate
  fib20               literal frequencies in Fibonacci proportion over 20
                      symbols.  zlib also finds matches among the frequent
                      symbols, and the tree stays within 15 bits; deep15 is
                      the case that does overflow
  deep15              match lengths in 17 length codes with counts 1.7 ** i: a
                      literal/length tree 17 deep, which gen_bitlen repairs
                      (the bit-length tree's repair at 7 is reached by several
                      cases)
  slide_nil           a string at window position 32768 exactly, matched from
                      65274 (distance MAX_DIST) after the slide made it
                      position 0, which is NIL
"""
import numpy as np

import compress_corpus as CC

FRAGS = (0, 1000, 4096, 65280, 65530)


def _far(dist, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 200, 100 + dist + 64 + 500, dtype=np.uint8)
    marker = rng.integers(200, 256, 64, dtype=np.uint8)
    a[100:164] = marker
    a[100 + dist:164 + dist] = marker
    return a.tobytes()


def _toofar(dist, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 200, 50 + dist + 300, dtype=np.uint8)
    a[50:53] = (250, 251, 252)
    a[50 + dist:53 + dist] = (250, 251, 252)
    a[53], a[53 + dist] = 1, 2
    return a.tobytes()


def _fib20():
    """Fibonacci counts 1, 1, 2, 3, ... over 20 symbols, shuffled (17710
    bytes).  The frequent symbols also form matches, so the tree zlib builds
    is shallower than the literal counts alone would make it (see deep15)."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(20)
    syms = np.concatenate([np.full(f, 33 + k, dtype=np.uint8) for k, f in enumerate(fib)])
    rng.shuffle(syms)
    return syms.tobytes()


def _deep15():
    """A block whose literal/length tree is 17 deep before the repair: after
    32766 random bytes (two blocks of literals), 11805 matches in one block
    whose lengths fall in 17 length codes with counts round(1.7 ** i) -- each
    count more than all smaller ones together, so Huffman's tree is one long
    chain.  Every match copies 5..62 bytes from 300..32000 back; a copy never
    starts with the byte that would extend the match before it, which keeps
    stray literals and shorter matches (a few of them at the bottom of the
    tree break the chain) out of the block."""
    lens_of_code = [5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 21, 25, 29, 33, 38, 46, 54]
    counts = [int(round(1.7 ** i)) for i in range(17)][::-1]  # the shortest is the most frequent
    rng = np.random.default_rng(20)
    lens = np.concatenate([np.full(c, lens_of_code[i]) for i, c in enumerate(counts)])
    rng.shuffle(lens)
    buf = bytearray(rng.integers(0, 256, 32766, dtype=np.uint8).tobytes())
    follow = -1
    for ln in lens:
        while True:
            p = len(buf) - int(rng.integers(300, 32000))
            if follow < 0 or buf[p] != buf[follow]:
                break
        buf += buf[p:p + int(ln)]
        follow = p + int(ln)
    return bytes(buf)


def _slide_nil(seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 200, 65274 + 64 + 5000, dtype=np.uint8)
    marker = rng.integers(200, 256, 64, dtype=np.uint8)
    a[32768:32768 + 64] = marker
    a[65274:65274 + 64] = marker
    return a.tobytes()


def named_cases():
    """[(name, bytes)], every payload at most 300 KB"""
    out = [(f"len{n}", CC.text(n, 100 + n)) for n in (0, 1, 2, 3, 4, 261, 262, 263)]
    out += [(f"far{d}", _far(d, d)) for d in (32506, 32507, 32768)]
    for n in (65273, 65274, 65275, 65276, 65277, 65535, 65536, 65537,
              131069, 131070, 131071, 131072, 131073, 131074, 131075):
        out.append((f"text{n}", CC.text(n, n)))
    out += [("rand20000", CC.random_bytes(20000, 11)), ("text40", CC.text(40, 40)),
            ("run300k", b"\x07" * 300_000), ("period8", bytes(range(8)) * (300_000 // 8)),
            ("toofar4096", _toofar(4096, 12)), ("toofar4097", _toofar(4097, 13)),
            ("abcabcabc", b"abcabcabc"), ("fib20", _fib20()), ("deep15", _deep15()), ("slide_nil", _slide_nil(14)),
            ("json100k", CC.json_like(100_000, 15)), ("low150k", CC.low_entropy(150_000, 5))]
    return out


def cases():
    """the named cases, then compress_corpus.py's (prefixed cc_)"""
    return named_cases() + [("cc_" + n, d) for n, d in CC.cases()]


def random_inputs(seed, count):
    """[(bytes, frag)]: seeded inputs of mixed kinds and sizes, each with a
    random fragment size"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        kind = int(rng.integers(0, 6))
        n = int(rng.choice([0, 1, 5, 40, 300, 1000, 3000, 9000, 30000, 70000], p=[.02, .03, .05, .1, .2, .2, .2, .1, .07, .03]))
        n = int(rng.integers(n // 2, n + 1)) if n > 1 else n
        s = int(rng.integers(0, 1 << 31))
        if kind == 0:
            b = CC.text(n, s)
        elif kind == 1:
            b = CC.random_bytes(n, s)
        elif kind == 2:
            b = CC.low_entropy(n, s)
        elif kind == 3:
            b = CC.json_like(n, s)
        elif kind == 4:
            b = CC.mostly_random(n, s)
        else:
            p = CC.random_bytes(int(rng.integers(1, 40)), s)
            b = (p * (n // len(p) + 1))[:n]
        # the interface's fragmentation: equal fragments of `frag` bytes and a
        # shorter last one (0: one fragment); at most a few thousand of them
        top = int(rng.choice([3, 64, 300, 5000, 70000]))
        frag = int(rng.integers(max(1, n // 3000), max(top, n // 3000 + 1) + 1)) if rng.integers(0, 8) else 0
        out.append((b, frag))
    return out


if __name__ == "__main__":
    # python tests/gzip_compress_corpus.py DIR: the named cases as files (the
    # input of tests/cpp/deflate_core_main.cpp)
    import os
    import sys
    os.makedirs(sys.argv[1], exist_ok=True)
    for name, data in named_cases():
        with open(os.path.join(sys.argv[1], name + ".bin"), "wb") as f:
            f.write(data)
