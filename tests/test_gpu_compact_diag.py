"""Compaction on the diagnostic library variant in a child process
(tests/compact_diag_cases.py): the key table's tag cut to 4 bits, so that
different keys collide on a tag and the key comparison decides."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(case, **env):
    lib = os.path.join(ROOT, "redpanda_amd", "librpgpu_diag.so")
    assert os.path.exists(lib), "librpgpu_diag.so missing: __graft_entry__.build() builds it"
    e = dict(os.environ, RPGPU_VARIANT="diag", **env)
    r = subprocess.run([sys.executable, "-m", "tests.compact_diag_cases", case], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_tag_collisions_are_settled_by_key_bytes():
    assert "short_tag ok" in _run("short_tag", RPGPU_CKEY_TAG_BITS="4")
