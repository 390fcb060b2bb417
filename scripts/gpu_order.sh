# The full bench's stanzas (c1,h2d,c2,c5,c6) under two side-stream
# setups (diagnostics): the product, and the diagnostic build with the side
# stream at default priority (RPGPU_SIDE_PRIO=0)
set -e
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
run() {
timeout -k 10 600 env $3 python -u bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/ord_$2.json 2> $OUT/ord_$2.err || { tail -5 $OUT/ord_$2.err; exit 1; }
python3 - $OUT/ord_$2.json $2 <<'PY'
import json,sys
j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); c=j['config']
print(sys.argv[2], 'c1', j['ms_per_step'])
for k in ('c2','c5','c6'):
    if k in c: print(sys.argv[2], k, c[k]['ms_per_step'], c[k]['stage_ms'].get('resolve_plan'), c[k]['stage_ms'].get('decode'))
PY
}
run x prio "RPGPU_X=1"
run x noprio "RPGPU_VARIANT=diag RPGPU_SIDE_PRIO=0"
