"""Golden vectors of the gzip compressor: length + sha256 of what zlib gives
through gzip_compressor::compress's call pattern (deflateInit2(-1, DEFLATED,
15 + 16, 8, default strategy), one deflate(Z_NO_FLUSH) per fragment,
Z_FINISH), driven here through Python's zlib, on the named cases of
tests/gzip_compress_corpus.py at its fragment sizes.  The zlib version is
recorded: the bytes are those of zlib 1.2.11.  They pin the device
(tests/test_gpu_deflate.py) where no zlib of that version can be relied on.
Run: python tests/golden/make_gzip_golden.py"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gzip_compress_corpus as G  # noqa: E402


def zlib_gzip(data, frag):
    c = zlib.compressobj(-1, zlib.DEFLATED, 31, 8, 0)
    step = frag or len(data) or 1
    return b"".join(c.compress(data[f:f + step]) for f in range(0, len(data), step)) + c.flush()


if __name__ == "__main__":
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    vec = {}
    for name, data in G.named_cases():
        for frag in G.FRAGS:
            r = zlib_gzip(data, frag)
            vec[f"{name}/{frag}"] = [len(r), hashlib.sha256(r).hexdigest()]
    with open(os.path.join(HERE, "gzip_compress_vectors.json"), "w") as f:
        json.dump({"zlib": zlib.ZLIB_RUNTIME_VERSION, "vectors": vec}, f, indent=0, sort_keys=True)
    print(len(vec), "vectors")
