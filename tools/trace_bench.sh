#!/bin/bash
# Runs ON the GPU box: rocprofv3 kernel trace of a short headline bench, per-kernel summary to $OUT/trace_<tag>.md
TAG=${1:-x}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-tools/_tmp}  # traces, logs and summaries (relative to the repository root)
mkdir -p $OUT/prof
rocprofv3 --kernel-trace --stats -d $OUT/prof -o t_${TAG} -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary > $OUT/prof/t_${TAG}.log 2>&1
python tools/rocpd_stats.py $OUT/prof/t_${TAG}_results.db > $OUT/trace_${TAG}.md
rm -f $OUT/prof/t_${TAG}_results.db
head -40 $OUT/trace_${TAG}.md
grep -h '"metric"' $OUT/prof/t_${TAG}.log | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['phases_ms'])"
