"""bench.py's own control flow, on the CPU (no GPU): round 3's headline bench
shipped with a name deleted that its function never bound, and its N > 1
branch had never executed anywhere.

1. A static check over bench.py and the host modules it drives: every name a
   function reads or `del`s must be bound somewhere visible to it.
2. The whole bench (C1 headline, the C2 / C5 / C6 stanzas, CPU baselines,
   segment index, gather check) runs through `bench.main` with a CPU stand-in
   platform whose engine is the oracle (test infrastructure standing in for
   the device: this exercises the bench's logic, not the kernels).
3. The N > 1 path: two gloo ranks run `bench.main` with --gather records and
   --check-gather; rank 0's gathered job must equal one job over every
   partition.
"""
import ast
import builtins
import io
import json
import os
import socket
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = ["bench.py", "__graft_entry__.py", "redpanda_amd/shard.py", "redpanda_amd/engine.py",
           "redpanda_amd/_lib.py", "redpanda_amd/build.py"]

_SCOPES = (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda, ast.ClassDef, ast.ListComp, ast.SetComp, ast.DictComp,
           ast.GeneratorExp)


def _direct(node):
    """Nodes of `node`'s own scope (nested scopes are not descended into,
    but are yielded themselves)."""
    for child in ast.iter_child_nodes(node):
        yield child
        if not isinstance(child, _SCOPES):
            yield from _direct(child)


def _bound(scope):
    names = set()
    if isinstance(scope, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
        a = scope.args
        for arg in a.posonlyargs + a.args + a.kwonlyargs + [x for x in (a.vararg, a.kwarg) if x]:
            names.add(arg.arg)
    if isinstance(scope, (ast.ListComp, ast.SetComp, ast.DictComp, ast.GeneratorExp)):
        for g in scope.generators:
            names |= {n.id for n in ast.walk(g.target) if isinstance(n, ast.Name)}
    for n in _direct(scope):
        if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
            names.add(n.id)
        elif isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            names.add(n.name)
        elif isinstance(n, (ast.Import, ast.ImportFrom)):
            names |= {(a.asname or a.name).split(".")[0] for a in n.names}
        elif isinstance(n, (ast.Global, ast.Nonlocal)):
            names |= set(n.names)
        elif isinstance(n, ast.ExceptHandler) and n.name:
            names.add(n.name)
    return names


def unbound_names(src: str, fname: str = "<src>"):
    """[(line, name, 'read' | 'del')] for names a scope reads or deletes
    without any binding visible to it (flow-insensitive)."""
    tree = ast.parse(src, fname)
    module = _bound(tree) | {"__file__", "__name__", "__doc__", "__spec__", "__path__"}
    problems = []

    def visit(scope, visible):
        own = _bound(scope)
        for n in _direct(scope):
            if isinstance(n, ast.Name):
                if isinstance(n.ctx, ast.Del) and n.id not in own:
                    problems.append((n.lineno, n.id, "del"))
                elif isinstance(n.ctx, ast.Load) and n.id not in own | visible | module and not hasattr(builtins, n.id):
                    problems.append((n.lineno, n.id, "read"))
        inner = visible if isinstance(scope, ast.ClassDef) else visible | own
        for n in _direct(scope):
            if isinstance(n, _SCOPES):
                visit(n, inner)
    visit(tree, set())
    return problems


def test_static_check_catches_round3_bug():
    src = "def run_c1():\n    out = 1\n    del out, host_base\n"
    assert unbound_names(src) == [(3, "host_base", "del")]
    src = "def f(a):\n    g = lambda x: x + a + b\n    return [y for y in g(1)]\n"
    assert unbound_names(src) == [(2, "b", "read")]


@pytest.mark.parametrize("rel", CHECKED)
def test_no_unbound_names(rel):
    with open(os.path.join(ROOT, rel)) as f:
        assert unbound_names(f.read(), rel) == []


# ---------------------------------------------------------------------------
# CPU stand-in platform: the oracle plays the engine
# ---------------------------------------------------------------------------
TIMINGS = {"total": 2.0, "discover": 0.1, "resolve_plan": 0.2, "validate": 1.0, "decode": 0.5, "walk": 0.2}


class OracleEngine:
    """The Engine surface bench.py uses, over CPU tensors, computed by the
    oracle (rpo_run_job / rpo_segment_index)."""

    def __init__(self):
        from oracle import oracle as O
        self.O = O
        O.build()

    def alloc_outputs(self, n_segments, batch_capacity, record_capacity, decoded_capacity, bitmap=True):
        import torch
        from redpanda_amd import abi
        from redpanda_amd.engine import DeviceResult
        u8 = torch.uint8
        return DeviceResult(
            batches=torch.zeros(max(batch_capacity, 1) * abi.BATCH_RESULT.itemsize, dtype=u8),
            records=torch.zeros(max(record_capacity, 1) * abi.RECORD_INDEX.itemsize, dtype=u8),
            decoded=torch.zeros(max(decoded_capacity, 1), dtype=u8),
            summaries=torch.zeros(max(n_segments, 1) * abi.SEGMENT_SUMMARY.itemsize, dtype=u8),
            totals=torch.zeros(abi.JOB_TOTALS.itemsize, dtype=u8),
            bitmap=torch.zeros(((max(batch_capacity, 1) + 63) // 64) * 8, dtype=u8) if bitmap else None,
            n_segments=n_segments)

    def submit(self, data, seg_offsets, out, flags, chunk_bytes=0, stream=None, d_seg_offsets=None, **kw):
        import torch
        from redpanda_amd import abi
        offs = np.asarray(seg_offsets, dtype=np.uint64)
        bc = out.batches.numel() // abi.BATCH_RESULT.itemsize
        rc = out.records.numel() // abi.RECORD_INDEX.itemsize
        r = self.O.run_job(data[: int(offs[-1])].numpy(), offs, flags, batch_cap=bc, record_cap=rc,
                           decoded_cap=out.decoded.numel())
        for dst, src in ((out.batches, r.batches), (out.records, r.records), (out.decoded, r.decoded),
                         (out.summaries, r.summaries), (out.totals, np.asarray(r.totals)),
                         (out.bitmap, r.bitmap)):
            if dst is not None:
                b = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
                dst[: b.size] = torch.from_numpy(b.copy())
        return out

    def set_timing(self, on=True):
        pass

    def last_timings(self):
        return dict(TIMINGS)

    def segment_index(self, out, base_offsets, step=None, stream=None, outputs=None):
        import torch
        from redpanda_amd import abi
        h = out.to_host()
        step = step or abi.INDEX_DEFAULT_STEP
        ix = self.O.segment_index(h.batches, h.summaries, list(base_offsets), step=step)
        cap = max(out.batches.numel() // abi.BATCH_RESULT.itemsize, 1)
        st = np.zeros(max(out.n_segments, 1), dtype=abi.INDEX_STATE)
        ro, rt, ps = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        for k, (s, a, b, c) in enumerate(ix):
            st[k] = s
            f, n = int(s["first_entry"]), int(s["n_entries"])
            ro[f:f + n], rt[f:f + n], ps[f:f + n] = a, b, c
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        return t(st.view(np.uint8)), t(ro.view(np.int32)), t(rt.view(np.int32)), t(ps.view(np.int64))

    def validate_host(self, segments, flags):
        """rpgpu_validate_host's result: one job over the host segments."""
        from redpanda_amd import abi
        from redpanda_amd.engine import HostResult
        segs = [np.ascontiguousarray(x, dtype=np.uint8) for x in segments]
        offs = np.cumsum([0] + [x.size for x in segs]).astype(np.uint64)
        data = np.concatenate(segs)
        total = int(offs[-1])
        r = self.O.run_job(data, offs, flags, batch_cap=total // abi.HEADER_SIZE + len(segs) + 1,
                           record_cap=max(total // 4, 64), decoded_cap=1)
        return HostResult(r.batches, r.records, r.decoded[:0], r.summaries, r.totals, None)

    @staticmethod
    def index_to_host(states, rel_off, rel_time, pos, n_segments):
        from redpanda_amd import abi
        st = np.frombuffer(states.numpy().tobytes(), dtype=abi.INDEX_STATE)[:n_segments]
        ro, rt, ps = rel_off.numpy().view(np.uint32), rel_time.numpy().view(np.uint32), pos.numpy().view(np.uint64)
        return [(s, ro[int(s["first_entry"]):int(s["first_entry"]) + int(s["n_entries"])].copy(),
                 rt[int(s["first_entry"]):int(s["first_entry"]) + int(s["n_entries"])].copy(),
                 ps[int(s["first_entry"]):int(s["first_entry"]) + int(s["n_entries"])].copy()) for s in st]


class CpuPlatform:
    def __init__(self, local):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")

    def engine(self):
        return OracleEngine()

    def sync(self):
        pass

    def empty_cache(self):
        pass

    def comm_device(self, backend):
        return self.device

    def host_segments(self, data, seg_bytes, n):
        return [data[i * seg_bytes:(i + 1) * seg_bytes].numpy().copy() for i in range(n)]

    def time_on_side_stream(self, first, again, reps):
        t = time.perf_counter()
        res = first(None)
        for _ in range(reps):
            res = again(None, res)
        return (time.perf_counter() - t) * 1e3 / (reps + 1), res


def _small(bench):
    """Shrink the stanza workloads to oracle-friendly sizes (keeping C6's
    multi-partition CPU-sample branch)."""
    bench.C2_PARTS, bench.C2_SEG = 2, 3 << 20
    bench.C5_PARTS, bench.C5_SEG = 3, 2 << 20
    bench.C6_CPU_PARTS = 2
    bench.CPU_C1_SAMPLE = 1 << 20


def _run_bench(argv):
    sys.path.insert(0, ROOT)
    import bench
    _small(bench)
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main(argv, platform=CpuPlatform)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    return lines


@pytest.fixture
def env1(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("OMP_NUM_THREADS", "2")


def test_bench_single_rank_all_stanzas(env1, rplib, tmp_path):
    lines = _run_bench(["--full", "--steps", "1", "--warmup", "1", "--seg-gib", str(2 / 1024), "--partitions", "2",
                        "--detail-out", str(tmp_path / "detail.json")])
    assert len(lines) == 1
    # the driver keeps the last 8 KB of stdout: the whole line must fit well inside
    assert len(lines[0]) < 6000, len(lines[0])
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["value"] > 0
    assert j["config"]["parity"] == {"all_batches_valid": True, "bitmap_all_ones": True}
    assert j["roofline"]["frac"] > 0 and j["roofline"]["bound"] == "hbm"
    assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["cores"] >= 1
    assert "error" not in (j["config"]["segment_index"] or {})
    for name in ("c2", "c5", "c6"):
        st = j["config"][name]
        assert "error" not in st, (name, st)
        assert st["parity"]["batches"] > 0 and st["roofline"]["kernel_ms"] > 0
        assert st["cpu_baseline"] is not None
    assert j["config"]["c2"]["parity"]["all_valid"]
    assert j["config"]["c6"]["member_pass"]["decoded_bytes"] > 0
    h = j["config"]["h2d"]
    assert "error" not in h and h["GBps"] > 0 and h["parity"]["counts_and_flags_match"], h
    # the full stanzas (per-kernel tables) go to --detail-out
    d = json.load(open(tmp_path / "detail.json"))
    assert set(d) >= {"c1", "c2", "c5", "c6"} and "workload" in d["c2"]


def test_bench_stanza_failure_keeps_headline(env1, rplib, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    def boom(*a, **k):
        raise RuntimeError("stanza exploded")
    monkeypatch.setattr(bench, "run_compressed", boom)
    lines = _run_bench(["--full", "--steps", "1", "--warmup", "0", "--seg-gib", str(1 / 1024), "--partitions", "1",
                        "--no-cpu-baseline", "--workloads", "c1,c2"])
    j = json.loads(lines[0])
    assert j["value"] is not None and j["ms_per_step"] > 0 and "stanza exploded" in j["config"]["c2"]["error"]


PLAIN = ["--gpus", "1", "--steps", "2", "--warmup", "0", "--seg-gib", str(2 / 1024), "--partitions", "2"]


def test_bench_plain_run_is_lean(env1, rplib, monkeypatch):
    """Without --full only the headline runs: no stanza, host path, segment
    index or CPU baseline (each would raise here), and the line still carries
    the headline's fields -- also with no warm-up step."""
    sys.path.insert(0, ROOT)
    import bench

    def boom(*a, **k):
        raise AssertionError("a plain run left the headline's path")
    for leg in ("run_compressed", "run_h2d", "cpu_baseline_c1", "cpu_baseline_decode", "check_gather"):
        monkeypatch.setattr(bench, leg, boom)
    monkeypatch.setattr(CpuPlatform, "time_on_side_stream", boom)
    lines = _run_bench(PLAIN)
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["unit"] == "GB/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["steps"] == 2
    assert j["value"] > 0 and j["ms_per_step"] > 0
    # value = job bytes per step / time per step (the line rounds it to 0.01)
    assert j["value"] == pytest.approx(2 * (2 << 20) / (j["ms_per_step"] * 1e-3) / 1e9, rel=1e-3, abs=0.006)
    c = j["config"]
    assert c["parity"] == {"all_batches_valid": True, "bitmap_all_ones": True}
    assert not j["cpu_baseline"] and c["segment_index"] is None
    assert not {"h2d", "c2", "c5", "c6"} & set(c)
    assert j["roofline"]["kernel_ms"] > 0


@pytest.mark.parametrize("argv", [["--workloads", "c1,c2"], ["--check-gather"], ["--steps", "0"],
                                  ["--full", "--workloads", "c2", "--dump-outputs", "x"]])
def test_bench_rejects_options_that_need_more(argv):
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_bench_dump_outputs(env1, rplib, tmp_path, monkeypatch):
    """--dump-outputs: the last step's outputs as float32 / float64 .npy
    files that equal the oracle's job over the same seeded input, identical
    from run to run, sampled (same rows every run) above the caps."""
    sys.path.insert(0, ROOT)
    import bench
    import synth
    from redpanda_amd import abi
    monkeypatch.setattr(bench, "DUMP_RECORD_ROWS", 100)
    a, b = tmp_path / "a", tmp_path / "b"
    assert len(_run_bench(PLAIN + ["--dump-outputs", str(a)])) == 1
    assert len(_run_bench(PLAIN + ["--dump-outputs", str(b)])) == 1
    names = sorted(p.name for p in a.iterdir())
    assert names == ["batch_rows.npy", "batches.npy", "bitmap.npy", "record_rows.npy", "records.npy",
                     "summaries.npy", "totals.npy"]
    got = {n[:-4]: np.load(a / n) for n in names}
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n[:-4]], np.load(b / n)), n
    assert sum(x.nbytes for x in got.values()) < 64e6
    # the same job through the oracle
    segs = []
    for p in range(2):
        s = np.zeros(2 << 20, dtype=np.uint8)
        synth.gen_segment(s, p, **synth.C1)
        segs.append(s)
    offs = np.arange(3, dtype=np.uint64) * np.uint64(2 << 20)
    from oracle import oracle as O
    ref = O.run_job(np.concatenate(segs), offs, abi.JOB_CRC | abi.JOB_PARSE)
    nb, nr = len(ref.batches), len(ref.records)
    assert nb > 0 and nr > 100
    assert list(got["totals"][:2]) == [nb, nr]
    assert np.array_equal(got["batch_rows"], np.arange(nb))
    for k, f in enumerate(abi.BATCH_COMPARE_FIELDS):
        assert np.array_equal(got["batches"][:, k], ref.batches[f].astype(np.float64)), f
    rows = got["record_rows"].astype(np.int64)
    assert len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < nr
    for k, f in enumerate(abi.RECORD_COMPARE_FIELDS):
        assert np.array_equal(got["records"][:, k], ref.records[f][rows].astype(np.float64)), f
    for k, f in enumerate(abi.SUMMARY_COMPARE_FIELDS):
        assert np.array_equal(got["summaries"][:, k], ref.summaries[f].astype(np.float64)), f
    assert got["bitmap"].shape == (nb,) and np.all(got["bitmap"] == 1)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, gather, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1")
    lines = _run_bench(["--full", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--seg-gib", str(1 / 1024),
                        "--partitions", "2", "--dist-backend", "gloo", "--gather", gather, "--check-gather",
                        "--no-cpu-baseline"])
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(lines, f)


@pytest.mark.parametrize("gather", ["records", "bitmap"])
def test_bench_world2_gloo_gather_check(rplib, tmp_path, gather):
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(2, _free_port(), gather, str(tmp_path)), nprocs=2, join=True)
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    assert len(r0) == 1 and r1 == []
    j = json.loads(r0[0])
    assert j["n_gpus"] == 2 and j["value"] > 0
    c = j["config"]
    assert c["partitions_per_gpu"] == 2 and "gloo" in c["parallelism"]
    gc = c["gather_check"]
    assert gc["consistent"] and gc["partitions"] == 4 and gc["index"], gc
    if gather == "records":
        assert c["gathered_records"]["consistent"]
    assert c["segment_index"]["gathered_at_rank0"]["partitions"] == 4


def test_test_helpers_resolve_abi_names():
    """Attribute reads of the abi module by the GPU tests and the smoke exist
    (the -m gpu suite is the only other place that would notice)."""
    import re
    from redpanda_amd import abi
    for rel in ["tests/test_gpu_parity.py", "tests/diag_cases.py", "tests/test_shard.py", "__graft_entry__.py",
                "bench.py", "redpanda_amd/shard.py", "redpanda_amd/engine.py"]:
        with open(os.path.join(ROOT, rel)) as f:
            for name in set(re.findall(r"\babi\.([A-Za-z_][A-Za-z0-9_]*)", f.read())):
                assert hasattr(abi, name), (rel, name)
