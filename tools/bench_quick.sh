# short bench on the GPU box: the --full line without PMC passes, CPU baseline and layerwise
# comparison (ms/step, path roofline, per-kernel times); files go to $OUT (default out/)
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --pmc 0 --cpu-baseline-steps 0 --compare-layerwise 0 --steps ${STEPS:-30} ${BENCH_ARGS:-} > $OUT/qb.json 2> $OUT/qb.err || { tail -20 $OUT/qb.err; exit 1; }
python -c "
import json;d=json.loads(open('$OUT/qb.json').read().strip().splitlines()[-1])
r=d['roofline'];print('ms/step',d['ms_per_step'],'value',d['value'],'path frac',r['frac'],'path us',r['us_per_step'])
for k,v in r['per_kernel'].items(): print('  ',k,v['avg_us'],v['frac'],'in-step',v['in_step_span_us'])"
