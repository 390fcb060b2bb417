# Round check: the GPU suite, smoke, the full bench (line + --detail-out), then
# the driver's plain bench command under rocprofv3 --kernel-trace --stats
# (scripts/trace_summary.py reads its C1 launches).
set -e
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
TAG=${1:-r05a}
SKIP_TESTS=${SKIP_TESTS:-}
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
if [ -z "$SKIP_TESTS" ]; then
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1 || { tail -60 $OUT/pytest_$TAG.log; exit 1; }
tail -2 $OUT/pytest_$TAG.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1 || { tail -30 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
fi
timeout -k 10 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --detail-out $OUT/bench_detail_$TAG.json > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
wc -c $OUT/bench_$TAG.json
tail -c 400 $OUT/bench_$TAG.json
if [ -z "${NO_TRACE:-}" ]; then
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o $TAG --output-format csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/prof_bench_$TAG.json 2> $OUT/prof_$TAG.log || { tail -30 $OUT/prof_$TAG.log; exit 1; }
echo "trace ok"
fi
if [ -n "${AB:-}" ]; then
W=c2,c5 bash scripts/gpu_ab.sh ${TAG}ab cur $AB cur $AB
fi
