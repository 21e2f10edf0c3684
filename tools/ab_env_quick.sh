# interleaved A/B of environment settings on one GPU box; files go to $OUT (default out/):
# AB_ENVS="RS_X=0 RS_X=1" REPS=3 BENCH_ARGS="..." bash tools/ab_env_quick.sh
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
for rep in $(seq ${REPS:-3}); do
for e in ${AB_ENVS}; do
  env $e timeout -k 10 300 python bench.py --full --pmc 0 --cpu-baseline-steps 0 --compare-layerwise 0 --keras-line 0 --steps ${STEPS:-60} ${BENCH_ARGS:-} > $OUT/ab.json 2> $OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
  python -c "import json;d=json.loads(open('$OUT/ab.json').read().strip().splitlines()[-1]);q=d.get('step_ms_distribution') or {};print('$e'.ljust(24),'ms/step',d['ms_per_step'],'median',q.get('median'),'p90',q.get('p90'))"
done
done
