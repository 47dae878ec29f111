#!/bin/bash
# Placement study, step 3: every family of allocations with the two probes beside each pair (pure write of y; value stream + write
# of y) -- does the effect need the gathers?
#   gpurun --timeout 600 -- 'bash scripts/collect_placement3.sh r04_placement3'
set -o pipefail
TAG=${1:-r04_placement3}
REPO=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=$REPO/gpurun_out/$TAG
LAB=$REPO/scripts/bin/placement_lab5
rm -rf "$OUT"; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for i in 1 2; do
  timeout -k 10 120 "$LAB" 4 127 10000000 1 > "$OUT/probes$i.txt" 2> "$OUT/probes$i.err"; rc=$?; echo "probes $i: rc $rc"
  if [ $rc -ne 0 ]; then echo "stopping"; exit 1; fi
done
