#!/bin/bash
# usage: gpu_lds_probe.sh [out.txt]   (on the GPU box; build first: see the head of tools/lds_probe.hip)
# Runs the built tools/_bin/lds_probe once under its own time limit and keeps its table (profiles/lds_trips.md, Part 0).
out=${1:-${OUT_DIR:-results}/lds_probe.txt}
mkdir -p "$(dirname "$out")"
[ -x tools/_bin/lds_probe ] || { echo "tools/_bin/lds_probe is not built"; exit 2; }
timeout -k 10 120 tools/_bin/lds_probe > "$out" 2>&1
rc=$?
cat "$out"
exit $rc
