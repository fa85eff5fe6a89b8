#!/bin/bash
# Kernel-time table of the joint step under FST_MATH=f32 (the unfused conv-engine path), ON the GPU box from the repo root:
#   bash tools/f32_profile.sh   ->  $PROFILE_OUT/r04_f32_kernel_stats.csv   (PROFILE_OUT defaults to profile_out/; stops at the first
#   failure)
set -e
R=$(pwd); OUT=${PROFILE_OUT:-$R/profile_out}; mkdir -p $OUT; cd /tmp; export TMPDIR=/tmp; rm -rf /tmp/prof_f32
FST_MATH=f32 timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_f32 -- python3 $R/bench.py --plain --steps 3 --warmup 1 > $OUT/f32_stats.log 2>&1 < /dev/null
f=$(find /tmp/prof_f32 -name "*kernel_stats.csv" | head -1)
[ -n "$f" ]
cp "$f" $OUT/r04_f32_kernel_stats.csv && head -25 "$f" | cut -d, -f1-4 | cut -c1-150
