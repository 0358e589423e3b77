#!/bin/bash
# FETCH_SIZE / WRITE_SIZE passes (separate, counters only with --kernel-trace) over tools/s2_dgrad_pmc_one.py: the stride-2
# data gradient of D0.down at batch 64.  usage (GPU box, repo root): bash tools/s2_dgrad_traffic.sh <outdir>
set -u
OUT=$1
export TMPDIR=/tmp
ROOT=$(pwd)
mkdir -p "$OUT"
for c in FETCH_SIZE WRITE_SIZE; do
  (cd /tmp && timeout 200 rocprofv3 --kernel-trace --pmc $c --output-format csv -d "$ROOT/$OUT/$c" -o p -- python "$ROOT/tools/s2_dgrad_pmc_one.py" > "$ROOT/$OUT/$c.log" 2>&1)
done
python tools/pmc_summary.py "$OUT" k_conv_allclass k_conv_parity4 > "$OUT/traffic.txt" 2>&1
find "$OUT" -name "*.csv" -size +300k -delete
cat "$OUT/traffic.txt"
