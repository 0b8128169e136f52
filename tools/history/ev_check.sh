R=$(pwd)
OUT=${OUT:-$(mktemp -d)}
timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 > $OUT/b_ev.json 2> $OUT/b_ev.err || { tail -5 $OUT/b_ev.err; exit 1; }
python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(d['value'],d['ms_per_step'],d['roofline'])" $OUT/b_ev.json
cd $OUT
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_ev -o e -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/prof_ev.log 2>&1 || exit 1
grep -h "gcm_single" $OUT/prof_ev/*kernel_stats.csv | cut -c1-120
grep "^{" $OUT/prof_ev.log | python3 -c "import json,sys;d=json.loads(sys.stdin.read());print(d['roofline']['kernel_ms'],d['roofline']['open_kernel_ms'])"
