"""storage::internal::compact_segment (include/rpgpu_redpanda.h) driven through
tests/cpp/compact_main.cpp, compared with the Python reference
(tests/compaction_ref.py)."""
import subprocess

import numpy as np
import pytest

from redpanda_amd import abi
from tests import compaction_ref as CR
from tests import test_compaction as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(rplib):
    import os
    from redpanda_amd import build as B
    # __graft_entry__.build() builds it; built here only when missing
    return B.COMPACT_BIN if os.path.exists(B.COMPACT_BIN) else B.build_compact_test()


def run(driver, seg, tmp_path):
    src, dst = tmp_path / "in.seg", tmp_path / "out.seg"
    src.write_bytes(seg.tobytes())
    r = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    return r, (dst.read_bytes() if dst.exists() else b"")


def test_compact_segment_tiny(driver, oracle, tmp_path):
    seg = TC.tiny_segment(oracle)
    ref, _, _, _ = TC._ref_compact(oracle, [seg])
    r, out = run(driver, seg, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) if " " in l else (l, "") for l in r.stdout.splitlines())
    assert out == ref.out.tobytes()
    assert [int(x) for x in lines["kept"].split()] == ref.kept_offsets[0]
    assert [int(x) for x in lines["codecs"].split()] == [int(c) for c in ref.batches["codec"]]
    g = ref.segments[0]
    assert [int(x) for x in lines["stats"].split()] == [int(g[f]) for f in (
        "records_in", "records_kept", "batches_in", "batches_out", "batches_rewritten", "bytes_out")]


def test_compact_segment_throws_on_repeated_offsets(driver, oracle, tmp_path):
    seg = [c[1] for c in TC.quirk_segments(oracle) if c[2] == abi.COMPACT_OFFSETS][0]
    r, _ = run(driver, seg, tmp_path)
    assert r.returncode == 2 and r.stdout.startswith("error "), r.stdout + r.stderr
