#!/bin/bash
# usage: ab_libs.sh <out-prefix> "<bench args>" <lib1.so> <lib2.so> ...   (through gpurun)
# A/B of library builds (FUSMI_LIB), round-robin over 3 rounds in separate processes.
out=$1; args=$2; shift 2
outdir=${OUT_DIR:-results}
mkdir -p $outdir
for round in 1 2 3; do
  for lib in "$@"; do
    FUSMI_LIB=$PWD/$lib timeout -k 10 300 python bench.py --full --no-cpu --traffic none --both-geometries 0 --repeats 3 $args > $outdir/${out}_tmp.json 2>> $outdir/${out}.err || { echo "$lib failed"; tail -3 $outdir/${out}.err; continue; }
    python - "$lib" $round <<PY
import json,sys
d=json.load(open("$outdir/${out}_tmp.json"))
print("round %s %-28s [$args]: %.4f ms/step, kernel %.4f ms, value %.4g" % (sys.argv[2], sys.argv[1], d["ms_per_step"], d["roofline"]["avg_launch_ms"], d["value"]))
PY
  done
done
