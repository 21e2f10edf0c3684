# round-end refresh on the GPU box: the --full bench line (with PMC traffic + cpu baseline),
# rocprof kernel stats of the bench, and the isolated north-star path; files go to $OUT
# (default out/)
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 600 python bench.py --full > $OUT/bench.log 2>&1 || { echo "bench failed"; tail -20 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log > $OUT/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o run --output-format csv -- python bench.py --steps 10 --warmup 3 > $OUT/prof_bench.log 2>&1 || { echo "rocprof failed"; exit 1; }
timeout -k 10 300 python benchmarks/bench_kernels.py --only dlrm_path > $OUT/path.jsonl 2> $OUT/path.err || { tail -20 $OUT/path.err; exit 1; }
cat $OUT/path.jsonl
echo done
