# Round-6 final records on the GPU box: the --full bench line (100 steps), its short form
# (20 steps after 5), and the kernel stats of the bench under rocprofv3; files go to $OUT
# (default out/)
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 600 python3 bench.py --full --steps 100 --warmup 10 > $OUT/fin_bench.json 2> $OUT/fin_bench.err || { tail -5 $OUT/fin_bench.err; exit 1; }
timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 5 > $OUT/fin_bench20.json 2> $OUT/fin_bench20.err || { tail -5 $OUT/fin_bench20.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/fin_prof -o run --output-format csv -- python3 bench.py --steps 10 --warmup 3 > $OUT/fin_prof.log 2>&1 || { tail -5 $OUT/fin_prof.log; exit 1; }
