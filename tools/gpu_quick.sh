#!/bin/bash
# usage: gpu_quick.sh [bench args]   -- GPU tests + short bench summary (outputs in $OUT_DIR, default results/)
outdir=${OUT_DIR:-results}
mkdir -p $outdir
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $outdir/gpu_tests.log 2> $outdir/gpu_tests.err; tail -3 $outdir/gpu_tests.log
timeout -k 10 300 python bench.py --full --no-cpu "$@" > $outdir/bench_quick.log 2> $outdir/bench_quick.err
tail -1 $outdir/bench_quick.log | python -c "
import sys,json
d=json.loads(sys.stdin.read())
print('value %.4e  ms/step %.3f  stiff_ms %.4f  kfrac %.3f  stepfrac %.3f'%(d['value'], d['ms_per_step'], d['roofline']['avg_launch_ms'], d['roofline']['frac'], d['step_roofline']['frac_of_8TBps']))
print(d['kernel_ms_per_step'])" || tail -20 $outdir/bench_quick.log
