#!/bin/bash
# refresh of the bench-derived profile files (K1 sources unchanged: the PMC traffic file stays valid)
R=$(cd "$(dirname "$0")/../.." && pwd); TAG=r02; export TMPDIR=/tmp; OUT_DIR=$(realpath -m "${OUT_DIR:-session_out}"); mkdir -p $OUT_DIR/prof
timeout 900 python bench.py --full --steps 50 --warmup 5 2>$OUT_DIR/bench_image.err | tail -1 > $OUT_DIR/${TAG}_bench_image.json
timeout 600 python bench.py --full --steps 50 --warmup 5 --kind psd --cpu-budget 0 --no-legs 2>&1 | tail -1 > $OUT_DIR/${TAG}_bench_psd.json
( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof/stats -o bench -- python $R/bench.py --full --steps 20 --warmup 3 --cpu-budget 0 > $OUT_DIR/prof/stats.log 2>&1 )
python tools/prof_summary.py stats $OUT_DIR/prof/stats/bench_results.db > $OUT_DIR/${TAG}_bench_kernel_stats.txt
python tools/bench_firbank.py > $OUT_DIR/${TAG}_banks.json 2>/dev/null
cut -c1-200 $OUT_DIR/${TAG}_banks.json
