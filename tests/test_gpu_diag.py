"""GPU cases run on the diagnostic library variant in a child process
(tests/diag_cases.py): the gzip / zstd first-pass pool exhausted by hostile
ISIZE trailers, RPGPU_JOB_HOST_CODECS without a loadable libzstd, and the
LZ4 fast-path record pool cut so that listed and walked blocks mix, zstd
ring-mode members through the wave decoder alone, each alternative launch
path a diagnostic switch still selects, and the split and compose CRC paths at
small shapes, with the counts that show they ran."""
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
    r = subprocess.run([sys.executable, "-m", "tests.diag_cases", case], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_member_pool_exhausted_hostile_isize():
    assert "small_pool ok" in _run("small_pool", RPGPU_INF_POOL_KIB="64")


def test_host_codec_missing_is_unsupported():
    assert "host_codec_missing ok" in _run("host_codec_missing", RPGPU_HOST_CODEC_MISSING="1")


@pytest.mark.parametrize("cap", ["0", "30000", "400000"])
def test_lz4_fast_pool_exhausted(cap):
    """a fast-path record pool too small for the job's
    LZ4 blocks (none / a few groups / most of them listed)."""
    assert "small_frec ok" in _run("small_frec", RPGPU_FREC_CAP=cap)


def test_zstd_ring_exact_wave_decoder():
    assert "zstd_ring_wave ok" in _run("zstd_ring_wave", RPGPU_ZS_FAST="0")


@pytest.mark.parametrize("switch", ["RPGPU_XXH_SIDE", "RPGPU_CRC_COMPOSE", "RPGPU_DCHAIN", "RPGPU_GZS", "RPGPU_LZF"])
def test_path_switch_off_matches_oracle(switch):
    """The launch-path switches that stay: each alternative path
    on one small job of every codec."""
    assert f"path_switch {switch}=0 ok" in _run("path_switch", **{switch: "0"})


def test_crc_split_small_shapes():
    """k_crc_split / k_crc_combine on payloads from 1 KiB (RPGPU_SPLIT_MIN_KIB=1);
    the diagnostic build's split count shows that they ran."""
    out = _run("crc_split_small", RPGPU_SPLIT_MIN_KIB="1")
    print(out.strip())
    assert "crc_split_small ok" in out


def test_crc_compose_small_shapes():
    """k_crc_compose on frames of two raw blocks around short and long gaps;
    the diagnostic build's compose count shows that it ran."""
    out = _run("crc_compose_small")
    print(out.strip())
    assert "crc_compose_small ok" in out
