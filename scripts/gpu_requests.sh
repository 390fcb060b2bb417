# Memory-side request counts of the C1 job's kernels (k_validate, k_walk,
# k_finalize_bitmap, ...): PMC-only rocprofv3 passes, no tracing in the same
# run, every pass bounded.  The L2 -> fabric request counters
# (TCC_EA0_RDREQ_sum / TCC_EA0_WRREQ_sum) in one pass, their 32-B / 64-B
# splits in a second one where `rocprofv3 -L` lists them.
# scripts/parse_requests.py TAG turns the passes into profiles/walk_requests.json.
# RPGPU_VARIANT=name profiles librpgpu_<name>.so (scripts/build_exp.py).
set -e
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-req}
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
BENCH="python3 bench.py --full --workloads c1 --steps 2 --warmup 1 --no-cpu-baseline --no-index"
timeout -k 10 120 rocprofv3 -L > $OUT/counters_$TAG.txt 2>&1
timeout -s KILL 300 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum -d $OUT/pmc_req_${TAG} -o r --output-format csv -- $BENCH > $OUT/pmc_req_${TAG}.log 2>&1
echo "requests ok"
SPLIT=""
for c in TCC_EA0_RDREQ_32B_sum TCC_EA0_WRREQ_64B_sum; do
grep -qw $c $OUT/counters_$TAG.txt && SPLIT="$SPLIT $c"
done
if [ -n "$SPLIT" ]; then
timeout -s KILL 300 rocprofv3 --pmc $SPLIT -d $OUT/pmc_reqsplit_${TAG} -o r --output-format csv -- $BENCH > $OUT/pmc_reqsplit_${TAG}.log 2>&1
echo "split ok:$SPLIT"
else
echo "no 32-B / 64-B split counters listed"
fi
