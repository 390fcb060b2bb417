"""Compaction cases that need the diagnostic library variant
(librpgpu_diag.so); tests/test_gpu_compact_diag.py runs each in a child
process with RPGPU_VARIANT=diag:

    python -m tests.compact_diag_cases <case>

exit status 0 = the case held; anything else prints why.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from redpanda_amd import abi  # noqa: E402


def case_short_tag():
    """RPGPU_CKEY_TAG_BITS=4: sixteen tag values for 31 keys per segment, so
    records of different keys meet on one tag and only the comparison of the
    key bytes keeps them apart.  A wrong match there would silently drop a
    record: the mixed case must still equal the reference, and the path must
    have run (key_compare_mismatches > 0)."""
    from oracle import oracle as O
    from redpanda_amd.engine import Engine
    from tests import test_compaction as TC
    assert os.environ.get("RPGPU_CKEY_TAG_BITS") == "4", "run with RPGPU_CKEY_TAG_BITS=4"
    O.build()
    eng = Engine(0)
    got, ref, _, _ = TC.run_device(eng, O, TC.mixed_segments(O))
    TC.assert_parity(got, ref)
    n = int(got.totals["key_compare_mismatches"])
    assert n > 0, "no tag collision was resolved by a key comparison"
    assert [int(s) for s in got.segments["status"]] == [abi.COMPACT_OK, abi.COMPACT_OK, abi.COMPACT_NOT_CLEAN]
    print(f"short_tag ok: {len(got.batches)} batches out, {n} key compare mismatches")


CASES = {"short_tag": case_short_tag}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
