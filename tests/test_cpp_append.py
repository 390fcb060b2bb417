"""kafka::produce_append (include/rpgpu_redpanda.h) driven through
tests/cpp/append_main.cpp, compared with the Python reference
(tests/append_ref.py): the log bytes, the error codes and the offsets."""
import struct
import subprocess

import pytest

from redpanda_amd import abi
from tests import append_ref as AR
from tests import test_append as TA

pytestmark = pytest.mark.gpu

# kafka/protocol/errors.h
ERROR_CODE = {abi.APPEND_OK: 0, abi.APPEND_CORRUPT_MESSAGE: 2, abi.APPEND_INVALID_RECORD: 87, abi.APPEND_MALFORMED: 2}


@pytest.fixture(scope="module")
def driver(rplib):
    import os
    from redpanda_amd import build as B
    # __graft_entry__.build() builds it; built here only when missing
    return B.APPEND_BIN if os.path.exists(B.APPEND_BIN) else B.build_append_test()


def run(driver, oracle, tmp_path, sets, nxt, times, all_batches):
    req = struct.pack("<I", len(sets))
    for s, n, t in zip(sets, nxt, times):
        req += struct.pack("<qqQ", n, t, len(s)) + bytes(s)
    src, dst = tmp_path / "request.bin", tmp_path / "log.bin"
    src.write_bytes(req)
    r = subprocess.run([driver, str(src), str(dst)] + (["--all"] if all_batches else []), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data, offs = TA.concat(sets)
    ref = AR.expected(oracle, data, offs, nxt, times, all_batches)
    assert dst.read_bytes() == ref.out.tobytes()
    lines = [l.split() for l in r.stdout.splitlines()]
    assert len(lines) == len(sets) and all(l[0] == "set" for l in lines)
    for l, g in zip(lines, ref.sets):
        assert [int(x) for x in l[1:]] == [ERROR_CODE[int(g["status"])], int(g["status"]), int(g["base_offset"]),
                                           int(g["last_offset"]), int(g["bytes_out"])]
    return ref


@pytest.mark.parametrize("all_batches", [False, True])
def test_produce_append_tiny(driver, oracle, tmp_path, all_batches):
    ct = abi.APPEND_CREATE_TIME
    ref = run(driver, oracle, tmp_path, TA.tiny_sets(), [0, 1 << 40, 1 << 62], [ct, ct, AR.TS0 + 5], all_batches)
    assert int(ref.sets["n_batches"][2]) == (2 if all_batches else 1)


@pytest.mark.parametrize("all_batches", [False, True])
def test_produce_append_verdicts(driver, oracle, tmp_path, all_batches):
    cases = TA.verdict_sets()
    ref = run(driver, oracle, tmp_path, [c[1] for c in cases], list(range(100, 100 + len(cases))),
              [abi.APPEND_CREATE_TIME] * len(cases), all_batches)
    assert [int(x) for x in ref.sets["status"]] == [c[3 if all_batches else 2] for c in cases]
