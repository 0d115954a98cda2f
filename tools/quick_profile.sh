#!/bin/bash
# One batch size, quickly: the bench line (family table) and the rocprofv3 kernel-trace table of the serial schedule.
#   tools/quick_profile.sh <batch> [steps] [output dir, default profile_out/quick]        (from the repo root)
B=${1:-32}; ST=${2:-6}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${3:-profile_out/quick}
cd /tmp && export TMPDIR=/tmp; cd $R
mkdir -p $OUT
python bench.py --full --no-extra-configs --batch-size $B --cpu-iters 0 --steps $ST --warmup 3 > $OUT/bench_bs$B.json 2>/dev/null
rm -rf /tmp/p1; timeout 600 rocprofv3 --kernel-trace -d /tmp/p1 -o x -- python bench.py --no-extra-configs --batch-size $B --cpu-iters 0 --steps $ST --warmup 4 --no-trace --serial > /dev/null 2>&1
python tools/rocpd_stats.py $(find /tmp/p1 -name "*.db" | head -1) $ST > $OUT/kernel_stats_bs${B}_serial.txt 2>&1
python - <<PY
import json
r=json.loads(open('$OUT/bench_bs$B.json').read().strip().splitlines()[-1])
print(r['ms_per_step'], json.dumps(r['kernel_time_ms_per_step']))
PY
head -40 $OUT/kernel_stats_bs${B}_serial.txt
